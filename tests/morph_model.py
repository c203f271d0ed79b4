"""The numpy model of voxel morphology (include/tdt_rt.h tdt_octree_morph / tdt_octree_extract_morph), the yardstick of the GPU
tests: every step on the Morton-sorted voxel list, neighbours by np.searchsorted on Morton keys.  numpy only."""
import numpy as np

from test_gpu_region_edit import inside
from tdt4230_project_raytracing_amd import rt

DILATE, ERODE, OPEN, CLOSE, SHELL = rt.MORPH_DILATE, rt.MORPH_ERODE, rt.MORPH_OPEN, rt.MORPH_CLOSE, rt.MORPH_SHELL


def offsets(connectivity):
    """[(t, d)] in ascending t(d) = 9 (dx + 1) + 3 (dy + 1) + (dz + 1): all 26 offsets, or the 6 faces."""
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                n = abs(dx) + abs(dy) + abs(dz)
                if n and (connectivity == 26 or n == 1):
                    out.append((9 * (dx + 1) + 3 * (dy + 1) + dz + 1, (dx, dy, dz)))
    return out


def _spread3(v):
    """10 bits -> every third bit, by magic masks (test_gpu_region_edit.morton, which this must equal, goes bit by bit: too
    slow for the millions of voxels of the large scenes)."""
    v = np.asarray(v).astype(np.int64)
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def _keys(xyz):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return (_spread3(xyz[:, 0]) << 2) | (_spread3(xyz[:, 1]) << 1) | _spread3(xyz[:, 2])


def _sorted(v):
    v = np.asarray(v, np.int32).reshape(-1, 4)
    k = _keys(v[:, :3])
    return np.ascontiguousarray(v) if (k[1:] >= k[:-1]).all() else np.ascontiguousarray(v[np.argsort(k, kind="stable")])


# Morton keys are spread3(x) << 2 | spread3(y) << 1 | spread3(z): one axis' bits moved by +-1 without decoding (dilated
# integer arithmetic: set / clear the other axes' bits so that the carry / borrow runs through them)
_ALL = (1 << 30) - 1
_AXIS = [sum(1 << (3 * b + s) for b in range(10)) for s in (2, 1, 0)]


def _shift_keys(keys, d):
    k = keys
    for a in range(3):
        m = _AXIS[a]
        if d[a] > 0:
            k = (((k | (_ALL ^ m)) + 1) & m) | (k & (_ALL ^ m))
        elif d[a] < 0:
            k = (((k & m) - 1) & m) | (k & (_ALL ^ m))
    return k


class _Probe:
    """Neighbour lookups in one sorted list S: per-axis face flags computed once, then one key shift and one searchsorted per
    offset."""

    def __init__(self, S, N):
        self.keys = _keys(S[:, :3])
        self.lo = [S[:, a] == 0 for a in range(3)]
        self.hi = [S[:, a] == N - 1 for a in range(3)]

    def __call__(self, d):
        """For every voxel p of S: (p + d is in the grid, p + d is in S, the key of p + d where it is in the grid)."""
        out = np.zeros(len(self.keys), bool)
        for a in range(3):
            if d[a]:
                out |= self.hi[a] if d[a] > 0 else self.lo[a]
        ok = ~out
        whole = not out.any()
        kq = _shift_keys(self.keys if whole else self.keys[ok], d)
        found = np.zeros(len(self.keys), bool)
        if len(kq):
            j = np.searchsorted(self.keys, kq)
            j[j == len(self.keys)] = 0
            hit = self.keys[j] == kq
            if whole:
                found = hit
            else:
                found[ok] = hit
        return ok, found, kq


def dilate_step(S, depth, connectivity, material):
    """D(S); S Morton-sorted {x, y, z, m}.  material < 0: a new q inherits from q + d for the first d in ascending t(d)."""
    S = np.asarray(S, np.int32).reshape(-1, 4)
    N = 1 << depth
    probe = _Probe(S, N)
    keys = probe.keys
    ck, ct, cm, cq = [], [], [], []
    for t, d in offsets(connectivity):                   # q = p - d is a candidate of p, which it sees through d: p = q + d
        e = tuple(-c for c in d)
        ok, found, kq = probe(e)
        new = np.flatnonzero(ok & ~found)
        ck.append(kq[~found[ok]])
        ct.append(np.full(len(new), t))
        cm.append(S[new, 3])
        cq.append(S[new, :3] + np.array(e, np.int32))
    ck, ct, cm, cq = np.concatenate(ck), np.concatenate(ct), np.concatenate(cm), np.concatenate(cq)
    if len(ck):
        order = np.lexsort((ct, ck))                     # by key, then by t
        first = order[np.concatenate([[True], ck[order][1:] != ck[order][:-1]])]
        new = np.concatenate([cq[first], cm[first][:, None]], 1).astype(np.int32)
        if material >= 0:
            new[:, 3] = material + 1
        S = np.concatenate([S, new])[np.argsort(np.concatenate([keys, ck[first]]), kind="stable")]
    return np.ascontiguousarray(S)


def erode_step(S, depth, connectivity, border):
    """E_b(S): the voxels all of whose neighbours are in S (or, b = 1, outside the grid)."""
    S = np.asarray(S, np.int32).reshape(-1, 4)
    N = 1 << depth
    probe = _Probe(S, N)
    keep = np.ones(len(S), bool)
    for _, d in offsets(connectivity):
        ok, found, _ = probe(d)
        keep &= (found | ~ok) if border else found
    return np.ascontiguousarray(S[keep])


def _repeat(step, chain, radius, *args):
    """`radius` steps from chain = (list, key, cache): cache (a dict, or None) maps the key of a chain of steps from V to its
    list, so the cases of one tree share their common prefixes (E, E.E, D, ...)."""
    S, key, cache = chain
    for _ in range(radius):
        if not len(S):
            break
        key = (key, step.__name__) + args
        if cache is None:
            S = step(S, *args)
        else:
            if key not in cache:
                cache[key] = step(S, *args)
            S = cache[key]
    return S, key, cache


def morph(V, depth, op, radius=1, connectivity=6, material=None, border=0, regions=None, cache=None):
    """The Morton-sorted voxel list tdt_octree_morph leaves / tdt_octree_extract_morph returns.  material None: inherit;
    regions None: no mask.  cache: a dict shared by calls on the SAME V (see _repeat)."""
    V = _sorted(V)
    mat = -1 if material is None else int(material)
    start = (V, "V", cache)
    if op == DILATE:
        R = _repeat(dilate_step, start, radius, depth, connectivity, mat)[0]
    elif op == ERODE:
        R = _repeat(erode_step, start, radius, depth, connectivity, border)[0]
    elif op == OPEN:
        R = _repeat(dilate_step, _repeat(erode_step, start, radius, depth, connectivity, 1), radius, depth, connectivity, mat)[0]
        R = V[np.isin(_keys(V[:, :3]), _keys(R[:, :3]))]     # a subset of V: the original materials
    elif op == CLOSE:
        R = _repeat(erode_step, _repeat(dilate_step, start, radius, depth, connectivity, mat), radius, depth, connectivity, 1)[0]
    elif op == SHELL:
        E = _repeat(erode_step, start, radius, depth, connectivity, border)[0]
        R = V[~np.isin(_keys(V[:, :3]), _keys(E[:, :3]))]
    else:
        raise ValueError(op)
    if regions is not None:
        regions = [regions] if isinstance(regions, rt.Region) else list(regions)
        R = np.concatenate([R[inside(R[:, :3], regions)], V[~inside(V[:, :3], regions)]])
    return _sorted(R)
