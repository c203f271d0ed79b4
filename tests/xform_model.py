"""The numpy model of tdt_octree_transform / tdt_octree_extract_transform (include/tdt_rt.h "affine transforms"): dense int64
arithmetic over the destination box, one voxel after the other in x slabs — s(p) for every p, then a look-up of S.  It knows
nothing of bricks, bit volumes or Morton ranges.  The builders below are the documented closed forms of include/tdt_host.h in
python integers."""
import numpy as np

from test_gpu_region_edit import inside, sort_vox

ONE = 65536
SLAB = 1 << 21                 # destination voxels evaluated at a time


class X:
    """The fields of struct tdt_xform as plain python: a (9), t (3), material (None: the source voxel's), dst_lo, dst_hi."""

    def __init__(self, a=(ONE, 0, 0, 0, ONE, 0, 0, 0, ONE), t=(0, 0, 0), material=None, dst_lo=(0, 0, 0), dst_hi=(2 ** 31 - 1,) * 3):
        self.a, self.t = [int(v) for v in a], [int(v) for v in t]
        self.material = material
        self.dst_lo, self.dst_hi = [int(v) for v in dst_lo], [int(v) for v in dst_hi]

    def with_(self, **kw):
        out = X(self.a, self.t, self.material, self.dst_lo, self.dst_hi)
        for k, v in kw.items():
            setattr(out, k, v)
        return out

    def fields(self):
        """What rt.Context.octree_transform takes."""
        return dict(a=self.a, t=self.t, material=self.material, dst_lo=self.dst_lo, dst_hi=self.dst_hi)


def source_of(x, p):
    """s(p) for (n, 3) int64 destination voxels: (a (2 p + 1) + t) >> 17, the shift arithmetic (a floor)."""
    q = 2 * np.asarray(p, np.int64) + 1
    a = np.array(x.a, np.int64).reshape(3, 3)
    return (q @ a.T + np.array(x.t, np.int64)) >> 17


def transform(V, depth, x, regions=None):
    """T as an (n, 4) int32 list, Morton-sorted.  regions None: S = V; a list (also an empty one): the voxels of V inside it."""
    N = 1 << depth
    V = np.asarray(V, np.int64).reshape(-1, 4)
    S = V if regions is None else V[inside(V[:, :3], regions)]
    lo = [max(v, 0) for v in x.dst_lo]
    hi = [min(v, N - 1) for v in x.dst_hi]
    if len(S) == 0 or any(l > h for l, h in zip(lo, hi)):
        return np.zeros((0, 4), np.int32)
    lin = (S[:, 0] * N + S[:, 1]) * N + S[:, 2]
    order = np.argsort(lin)
    lin, mat = lin[order], S[order, 3]
    ys, zs = np.arange(lo[1], hi[1] + 1), np.arange(lo[2], hi[2] + 1)
    step = max(1, SLAB // (len(ys) * len(zs)))
    out = []
    for x0 in range(lo[0], hi[0] + 1, step):
        xs = np.arange(x0, min(x0 + step, hi[0] + 1))
        p = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
        s = source_of(x, p)
        ok = ((s >= 0) & (s < N)).all(1)
        p, s = p[ok], s[ok]
        k = (s[:, 0] * N + s[:, 1]) * N + s[:, 2]
        at = np.minimum(np.searchsorted(lin, k), len(lin) - 1)
        hit = lin[at] == k
        m = mat[at[hit]] if x.material is None else np.full(int(hit.sum()), x.material + 1)
        out.append(np.concatenate([p[hit], m[:, None]], 1))
    return sort_vox(np.concatenate(out).astype(np.int32))


# ---- the documented closed forms: a = 65536 R^-1, t = 65536 (P - R^-1 P) -------------------------------------------------------
def about(rinv, pivot2, unit=ONE):
    """rinv: the inverse forward matrix as 3 x 3 integers over `unit` (Q16 entries = rinv * 65536 / unit must be whole)."""
    a = [[(ONE * v) // unit for v in row] for row in rinv]
    assert all((ONE * v) % unit == 0 for row in rinv for v in row)
    t = [ONE * pivot2[i] - sum(a[i][j] * pivot2[j] for j in range(3)) for i in range(3)]
    return X([v for row in a for v in row], t)


def identity():
    return X()


def translate(d):
    return X(t=[-int(v) * (1 << 17) for v in d])


def quarter_turns(axis, k, pivot2):
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k % 4]
    u, v = (axis + 1) % 3, (axis + 2) % 3
    r = [[0] * 3 for _ in range(3)]
    r[axis][axis] = 1
    r[u][u], r[u][v], r[v][u], r[v][v] = c, s, -s, c         # the transpose of the forward turn
    return about(r, pivot2, 1)


def mirror(axis, pivot2):
    r = [[1 if i == j else 0 for j in range(3)] for i in range(3)]
    r[axis][axis] = -1
    return about(r, pivot2, 1)


def scale(num, den, pivot2):
    a = [(2 * ONE * den[i] + num[i]) // (2 * num[i]) for i in range(3)]          # to nearest, halves up
    return X([a[0], 0, 0, 0, a[1], 0, 0, 0, a[2]], [(ONE - a[i]) * pivot2[i] for i in range(3)])


def rotation(axis, degrees, pivot):
    """The rounded closed form of a rotation about the line through `pivot` (continuous coordinates): Rodrigues in float64."""
    n = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    R = c * np.eye(3) + s * K + (1 - c) * np.outer(n, n)
    f = np.asarray(pivot, np.float64) - R @ np.asarray(pivot, np.float64)
    rinv = R.T
    return X(np.rint(ONE * rinv).astype(np.int64).ravel(), np.rint(-131072.0 * (rinv @ f)).astype(np.int64))
