"""The numpy model of the voxel smoothing unit (include/tdt_rt.h tdt_octree_smooth / tdt_octree_extract_smooth /
tdt_octree_density_field), the yardstick of the GPU tests.  Grids are indexed [x, y, z] and hold material + 1, 0 = empty, as in
tests/distance_model.py.  The density of a grid is taken chord by chord: a prefix sum along x turns the count of a chord of
half-length h into a difference of two entries, the prefix rows of all chords of one h are summed first (slices of an array
padded by R in y and z), and the two gathers per h clip the chord to the grid.  The support is the density of the full grid.
The nearest voxel of a new voxel is found by walking the ball's offsets in the header's order (|d|^2, dx, dy, dz), not through
distance_model.py, which tests/test_smooth_api.py compares it with.  numpy only."""
import functools

import numpy as np

from test_gpu_region_edit import inside
from tdt4230_project_raytracing_amd import rt
from distance_model import grid_of, list_of, window_of
from morph_model import _sorted

BOTH, ADD, REMOVE = rt.SMOOTH_BOTH, rt.SMOOTH_ADD, rt.SMOOTH_REMOVE
SPARSE = 64                      # at most this many set voxels: the nearest voxel by all pairs instead of the walk


@functools.lru_cache(None)
def chords(r2):
    """[(dy, dz, h)]: the x-chords of the ball, h = floor(sqrt(r2 - dy^2 - dz^2))."""
    R = window_of(r2)
    out = []
    for dy in range(-R, R + 1):
        for dz in range(-R, R + 1):
            rest = r2 - dy * dy - dz * dz
            if rest >= 0:
                h = 0
                while (h + 1) * (h + 1) <= rest:
                    h += 1
                out.append((dy, dz, h))
    return tuple(out)


def ball_size(r2):
    return sum(2 * h + 1 for _, _, h in chords(r2))


@functools.lru_cache(None)
def offsets(r2):
    """The ball's offsets sorted by (|d|^2, dx, dy, dz) as an (n, 3) array."""
    R = window_of(r2)
    d = [(dx * dx + dy * dy + dz * dz, dx, dy, dz) for dx in range(-R, R + 1) for dy in range(-R, R + 1) for dz in range(-R, R + 1)
         if dx * dx + dy * dy + dz * dz <= r2]
    return np.array(sorted(d), np.int64)[:, 1:]


_recent = {}                     # the last densities by (grid, r2): the cases of a test share their first step


def density(occ, r2):
    """d[x, y, z] = how many set voxels of occ the ball around (x, y, z) holds; nothing outside the grid is set.  (The result is
    shared between calls: read-only.)"""
    occ = np.asarray(occ, bool)
    key = (occ.shape, r2, occ.tobytes())
    if key not in _recent:
        if len(_recent) >= 4:
            _recent.pop(next(iter(_recent)))
        _recent[key] = _density(occ, r2)
        _recent[key].setflags(write=False)
    return _recent[key]


def _density(occ, r2):
    N = occ.shape[0]
    R = window_of(r2)
    P = np.zeros((N + 1, N + 2 * R, N + 2 * R), np.int32)                  # P[i] = the set voxels of a row with x < i
    np.cumsum(occ, axis=0, dtype=np.int32, out=P[1:, R:R + N, R:R + N])
    by_h = {}
    for dy, dz, h in chords(r2):
        rows = P[:, R + dy:R + dy + N, R + dz:R + dz + N]
        if h in by_h:
            by_h[h] += rows
        else:
            by_h[h] = rows.copy()
    x = np.arange(N)
    d = np.zeros((N, N, N), np.int32)
    for h, rows in by_h.items():
        d += rows[np.minimum(x + h + 1, N)] - rows[np.maximum(x - h, 0)]
    return d


@functools.lru_cache(None)
def support(N, r2):
    """n[x, y, z] = |(q + B) & G|: the density of the full grid."""
    n = density(np.ones((N, N, N), bool), r2)
    n.setflags(write=False)
    return n


def passes(d, n, threshold):
    """The threshold test T: threshold 0 / None = majority, otherwise a Q16 fraction of the support."""
    d, n = d.astype(np.int64), np.asarray(n, np.int64)
    return 2 * d > n if not threshold else 65536 * d >= threshold * n


def nearest_material(mat, new, r2):
    """The material + 1 of the nearest occupied voxel of every voxel of `new` (an (n, 3) array), by the header's order."""
    N = mat.shape[0]
    pts = np.argwhere(mat > 0)
    if len(pts) <= SPARSE:                                                   # a few voxels far apart: all pairs, the same order in one key
        out = np.zeros(len(new), np.int32)
        for i in range(0, len(new), 1 << 15):
            d = pts[None, :, :] - new[i:i + (1 << 15), None, :]
            d2 = (d * d).sum(2)
            assert (d2.min(1) <= r2).all(), "a new voxel has no voxel inside its ball"
            key = ((d2 * 64 + np.clip(d[:, :, 0], -32, 31) + 32) * 64 + np.clip(d[:, :, 1], -32, 31) + 32) * 64 + np.clip(d[:, :, 2], -32, 31) + 32
            p = pts[key.argmin(1)]
            out[i:i + (1 << 15)] = mat[p[:, 0], p[:, 1], p[:, 2]]
        return out
    out = np.zeros(len(new), np.int32)
    todo = np.arange(len(new))
    for o in offsets(r2):
        if not len(todo):
            break
        p = new[todo] + o
        ok = ((p >= 0) & (p < N)).all(1)
        m = np.zeros(len(todo), np.int32)
        m[ok] = mat[p[ok, 0], p[ok, 1], p[ok, 2]]
        out[todo[m > 0]] = m[m > 0]
        todo = todo[m == 0]
    assert not len(todo), "a new voxel has no voxel inside its ball"
    return out


def step(mat, r2, threshold=None, mode=BOTH, material=None, border=0, mask=None):
    """One step F on a grid of material + 1; mask: a bool grid (None: everywhere)."""
    occ = mat > 0
    N = mat.shape[0]
    t = passes(density(occ, r2), support(N, r2) if border else ball_size(r2), threshold)
    keep = t if mode == BOTH else (occ | t) if mode == ADD else (occ & t)
    if mask is not None:
        keep = np.where(mask, keep, occ)
    out = np.where(keep & occ, mat, 0).astype(np.int32)
    new = np.argwhere(keep & ~occ)
    if len(new):
        out[new[:, 0], new[:, 1], new[:, 2]] = material + 1 if material is not None and material >= 0 else nearest_material(mat, new, r2)
    return out


def mask_of(regions, N):
    """The union of the shapes as a bool grid, or None for no shapes."""
    regions = [regions] if isinstance(regions, rt.Region) else list(regions or ())
    if not regions:
        return None
    return inside(np.argwhere(np.ones((N, N, N), bool)), regions).reshape(N, N, N)


def smooth_grid(mat, radius2, iterations=1, threshold=None, mode=BOTH, material=None, border=0, regions=()):
    mask = mask_of(regions, mat.shape[0])
    for _ in range(iterations):
        nxt = step(mat, radius2, threshold, mode, material, border, mask)
        if np.array_equal(nxt, mat):
            break
        mat = nxt
    return mat


def smooth(V, depth, radius2, iterations=1, threshold=None, mode=BOTH, material=None, border=0, regions=()):
    """The Morton-sorted list tdt_octree_smooth leaves / tdt_octree_extract_smooth returns."""
    return _sorted(list_of(smooth_grid(grid_of(V, depth), radius2, iterations, threshold, mode, material, border, regions)))


def field(V, depth, lo, hi, radius2):
    """(density[z, y, x], support[z, y, x]) over the inclusive box, as tdt_octree_density_field returns them."""
    mat = grid_of(V, depth)
    s = tuple(slice(lo[a], hi[a] + 1) for a in range(3))
    d, n = density(mat > 0, radius2), support(mat.shape[0], radius2)
    return np.ascontiguousarray(d[s].transpose(2, 1, 0)).astype(np.int32), np.ascontiguousarray(n[s].transpose(2, 1, 0)).astype(np.int32)
