"""The numpy model of the exact Euclidean distance unit (include/tdt_rt.h tdt_octree_morph_round / tdt_octree_extract_morph_round /
tdt_octree_distance_field), the yardstick of the GPU tests.  Grids are indexed [x, y, z]; a voxel's RANK is its flat index
(x N + y) N + z, so a lower rank is a lexicographically lower (x, y, z).  Distance and nearest voxel travel as ONE int64 key
d2 * K + rank: the minimum of the keys is the smallest distance and, among equal distances, the lowest rank — the header's tie
rule — and because the key of a candidate is a sum over the axes, min-plus separates exactly.  numpy only."""
import numpy as np

from test_gpu_region_edit import inside
from tdt4230_project_raytracing_amd import rt
from morph_model import _sorted

DILATE, ERODE, OPEN, CLOSE, SHELL = rt.MORPH_DILATE, rt.MORPH_ERODE, rt.MORPH_OPEN, rt.MORPH_CLOSE, rt.MORPH_SHELL
SPARSE = 16                      # at most this many set voxels: all pairs instead of three passes


def window_of(r2):
    """The smallest integer R with R * R >= r2."""
    R = 1
    while R * R < r2:
        R += 1
    return R


def _K(N):
    return np.int64(N) ** 3


def _inf(N):
    return np.int64(1 << 20) * _K(N)          # above every real key: d2 <= 3 N^2 < 2^20 * ... for N <= 2^9


def transform(occ, R=None):
    """keys[x, y, z] = min over set voxels p of |q - p|^2 * K + rank(p), >= inf where occ has no voxel (within the window R per
    axis, when given: exact wherever d2 <= R^2).  Sparse sets: all pairs, whatever R."""
    occ = np.asarray(occ, bool)
    N = occ.shape[0]
    K, INF = _K(N), _inf(N)
    pts = np.argwhere(occ)
    if len(pts) <= SPARSE:
        ax = np.arange(N, dtype=np.int64)
        key = np.full((N, N, N), INF, np.int64)
        for p in pts:
            d2 = ((ax - p[0]) ** 2)[:, None, None] + ((ax - p[1]) ** 2)[None, :, None] + ((ax - p[2]) ** 2)[None, None, :]
            np.minimum(key, d2 * K + ((p[0] * N + p[1]) * N + p[2]), out=key)
        return key
    key = np.where(occ, np.arange(N ** 3, dtype=np.int64).reshape(N, N, N), INF)
    R = N - 1 if R is None else min(R, N - 1)
    for a in range(3):
        src = np.moveaxis(key, a, 0)
        out = src.copy()
        for o in range(1, R + 1):
            c = o * o * K
            np.minimum(out[:-o], src[o:] + c, out=out[:-o])      # the candidate at +o
            np.minimum(out[o:], src[:-o] + c, out=out[o:])       # the candidate at -o
        key = np.moveaxis(out, 0, a)
    return np.ascontiguousarray(key)


def split(key):
    """(d2, rank, found) of a key array."""
    N = key.shape[0]
    found = key < _inf(N)
    return np.where(found, key // _K(N), np.iinfo(np.int64).max), np.where(found, key % _K(N), -1), found


def brute(occ):
    """The all-pairs keys, for small grids: the definition itself."""
    occ = np.asarray(occ, bool)
    N = occ.shape[0]
    q = np.argwhere(np.ones_like(occ)).astype(np.int64)
    p = np.argwhere(occ).astype(np.int64)
    d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(2)
    return (d2 * _K(N) + ((p[:, 0] * N + p[:, 1]) * N + p[:, 2])[None, :]).min(1).reshape(N, N, N)


def ties(occ):
    """How many voxels have more than one set voxel at their minimum distance (small grids)."""
    occ = np.asarray(occ, bool)
    q = np.argwhere(np.ones_like(occ)).astype(np.int64)
    p = np.argwhere(occ).astype(np.int64)
    d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(2)
    return int(((d2 == d2.min(1)[:, None]).sum(1) > 1).sum())


def sparse_ties(V, depth):
    """ties() for a few voxels on a large grid: one pass per voxel keeps the minimum and how many voxels are at it."""
    N = 1 << depth
    ax = np.arange(N, dtype=np.int64)
    best = np.full((N, N, N), np.iinfo(np.int64).max, np.int64)
    count = np.zeros((N, N, N), np.int8)
    for p in np.asarray(V)[:, :3]:
        d2 = ((ax - p[0]) ** 2)[:, None, None] + ((ax - p[1]) ** 2)[None, :, None] + ((ax - p[2]) ** 2)[None, None, :]
        count = np.where(d2 < best, 1, count + (d2 == best)).astype(np.int8)
        np.minimum(best, d2, out=best)
    return int((count > 1).sum())


def grid_of(V, depth):
    """mat[x, y, z] = material + 1, 0 = empty."""
    N = 1 << depth
    V = np.asarray(V, np.int32).reshape(-1, 4)
    mat = np.zeros((N, N, N), np.int32)
    mat[V[:, 0], V[:, 1], V[:, 2]] = V[:, 3]
    return mat


def list_of(mat):
    p = np.argwhere(mat > 0)
    return _sorted(np.concatenate([p, mat[p[:, 0], p[:, 1], p[:, 2]][:, None]], 1).astype(np.int32))


def edge2(N):
    """The squared distance of every voxel to the nearest lattice point outside the grid."""
    ax = np.arange(N, dtype=np.int64)
    e = np.minimum(ax + 1, N - ax)
    return np.minimum(np.minimum(e[:, None, None], e[None, :, None]), e[None, None, :]) ** 2


def dilate(mat, r2, material=-1, capped=True):
    """D: new voxels within r2 of the set, with `material` or their nearest voxel's."""
    d2, rank, _ = split(transform(mat > 0, window_of(r2) if capped else None))
    new = (mat == 0) & (d2 <= r2)
    out = mat.copy()
    out[new] = material + 1 if material >= 0 else mat.reshape(-1)[rank[new]]
    return out


def erode(mat, r2, border, capped=True):
    """E_b: the voxels farther than r2 from every empty point (b = 0: and from the outside of the grid)."""
    d2 = split(transform(mat == 0, window_of(r2) if capped else None))[0]
    if not border:
        d2 = np.minimum(d2, edge2(mat.shape[0]))
    return np.where(d2 > r2, mat, 0)


def round_grid(mat, op, radius2, material=None, border=0, capped=True):
    m = -1 if material is None else int(material)
    if op == DILATE:
        return dilate(mat, radius2, m, capped)
    if op == ERODE:
        return erode(mat, radius2, border, capped)
    if op == SHELL:
        return np.where(erode(mat, radius2, border, capped) > 0, 0, mat)
    if op == OPEN:
        return np.where(dilate(erode(mat, radius2, 1, capped), radius2, m, capped) > 0, mat, 0)    # a subset of V: V's materials
    if op == CLOSE:
        return erode(dilate(mat, radius2, m, capped), radius2, 1, capped)
    raise ValueError(op)


def round_op(V, depth, op, radius2, material=None, border=0, regions=None):
    """The Morton-sorted list tdt_octree_morph_round leaves / tdt_octree_extract_morph_round returns.  regions None: no mask."""
    V = _sorted(V)
    R = list_of(round_grid(grid_of(V, depth), op, radius2, material, border))
    if regions is not None:
        regions = [regions] if isinstance(regions, rt.Region) else list(regions)
        R = np.concatenate([R[inside(R[:, :3], regions)], V[~inside(V[:, :3], regions)]])
    return _sorted(R)


def field(V, depth, lo, hi, max_d2, border=0):
    """(field[z, y, x], nearest[z, y, x, 3]) over the inclusive box, as tdt_octree_distance_field returns them."""
    mat = grid_of(V, depth)
    N = mat.shape[0]
    R = window_of(max_d2)
    d2, rank, _ = split(transform(mat > 0, R))
    if (mat > 0).sum() <= SPARSE:                 # the complement is dense: look around the few occupied voxels instead
        c2 = np.full(mat.shape, np.iinfo(np.int64).max, np.int64)
        for p in np.argwhere(mat > 0):
            w = tuple(slice(max(p[a] - R, 0), min(p[a] + R, N - 1) + 1) for a in range(3))
            ax = [np.arange(s.start, s.stop, dtype=np.int64) - p[a] for a, s in enumerate(w)]
            d2w = (ax[0] ** 2)[:, None, None] + (ax[1] ** 2)[None, :, None] + (ax[2] ** 2)[None, None, :]
            empty = mat[w] == 0
            if empty.any():
                c2[tuple(p)] = d2w[empty].min()
    else:
        c2 = split(transform(mat == 0, R))[0]
    if not border:
        c2 = np.minimum(c2, edge2(N))
    cap = max_d2 + 1
    occ = mat > 0
    f = np.where(occ, -np.minimum(c2, cap), np.minimum(d2, cap)).astype(np.int32)
    near = np.full((N, N, N, 3), -1, np.int32)
    ok = ~occ & (d2 <= max_d2)
    near[ok] = np.stack([rank[ok] // (N * N), rank[ok] // N % N, rank[ok] % N], 1)
    near[occ] = np.argwhere(occ)
    s = tuple(slice(lo[a], hi[a] + 1) for a in range(3))
    return np.ascontiguousarray(f[s].transpose(2, 1, 0)), np.ascontiguousarray(near[s].transpose(2, 1, 0, 3))
