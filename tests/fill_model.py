"""The numpy model of enclosed space (include/tdt_rt.h tdt_octree_extract_enclosed and its siblings), the yardstick of the GPU
tests: E(W, c) on a dense boolean grid by propagation from the grid's faces to a fixed point, the inherit rule along -x, the
mask.  The whole grid is held, so it serves depths up to 7; numpy only."""
import numpy as np

from morph_model import _keys, _sorted, offsets
from test_gpu_region_edit import inside
from tdt4230_project_raytracing_amd import rt


def grid_of(W, depth):
    """mat[x, y, z] = material + 1 of the wall voxel there, 0 where the grid is empty."""
    n = 1 << depth
    W = np.asarray(W, np.int64).reshape(-1, 4)
    mat = np.zeros((n, n, n), np.int16)
    mat[W[:, 0], W[:, 1], W[:, 2]] = W[:, 3]
    return mat


def outside(empty, connectivity):
    """The empty voxels on a face of the grid, grown through empty neighbours until nothing changes (nothing wraps)."""
    n = empty.shape[0]
    reach = np.zeros_like(empty)
    for a in range(3):
        for face in (0, n - 1):
            idx = [slice(None)] * 3
            idx[a] = face
            reach[tuple(idx)] = empty[tuple(idx)]
    offs = [d for _, d in offsets(connectivity)]
    while True:
        grown = reach.copy()
        for d in offs:
            src = tuple(slice(max(0, -s), n - max(0, s)) for s in d)      # p
            dst = tuple(slice(max(0, s), n - max(0, -s)) for s in d)      # p + d
            grown[dst] |= reach[src]
        grown &= empty
        if (grown == reach).all():
            return reach
        reach = grown


def outside_sweeps(empty, connectivity):
    """outside() for large grids (tools/fill_time.py: 256^3, 512^3): the same fixed point reached by whole-run sweeps.  A sweep
    along an axis carries reach through every run of empties in both directions (face neighbours, which connect under 26 too);
    one round is the six sweeps and, under 26, one step through all 26 offsets; it stops when a round changes nothing, i.e. when
    the set is closed under the full neighbourhood.  tests/test_fill_api.py pins it to outside()."""
    n = empty.shape[0]
    reach = np.zeros_like(empty)
    for a in range(3):
        for face in (0, n - 1):
            idx = [slice(None)] * 3
            idx[a] = face
            reach[tuple(idx)] = empty[tuple(idx)]
    diagonal = [d for _, d in offsets(26) if abs(d[0]) + abs(d[1]) + abs(d[2]) > 1] if connectivity == 26 else []
    while True:
        before = int(reach.sum())
        for a in range(3):
            r, e = np.moveaxis(reach, a, 0), np.moveaxis(empty, a, 0)     # views: the sweeps write reach itself
            for i in range(1, n):
                r[i] |= r[i - 1] & e[i]
            for i in range(n - 2, -1, -1):
                r[i] |= r[i + 1] & e[i]
        if diagonal:
            grown = reach.copy()
            for d in diagonal:
                src = tuple(slice(max(0, -s), n - max(0, s)) for s in d)
                dst = tuple(slice(max(0, s), n - max(0, -s)) for s in d)
                grown[dst] |= reach[src]
            reach = grown & empty
        if int(reach.sum()) == before:
            return reach


def enclosed_grid(W, depth, connectivity=6, fast=False):
    """E(W, c) as a boolean grid."""
    empty = grid_of(W, depth) == 0
    return empty & ~(outside_sweeps if fast else outside)(empty, connectivity)


def enclosed(W, depth, connectivity=6, material=None, regions=None, E=None, fast=False):
    """E(W, c) within the mask as a Morton-sorted list {x, y, z, material + 1}.  material None: each voxel takes the material of
    the first wall voxel met walking in decreasing x; regions None: no mask.  E: enclosed_grid(W, depth, connectivity), when the
    caller has it already (the propagation is the slow part)."""
    mat = grid_of(W, depth)
    n = 1 << depth
    if E is None:
        empty = mat == 0
        E = empty & ~(outside_sweeps if fast else outside)(empty, connectivity)
    p = np.argwhere(E)
    if material is None:
        # the x of the nearest wall at or below each x, per (y, z) row: a running maximum of the walls' own x
        at = np.where(mat > 0, np.arange(n, dtype=np.int16)[:, None, None], np.int16(-1))
        at = np.maximum.accumulate(at, axis=0)
        x = at[p[:, 0], p[:, 1], p[:, 2]]
        assert (x >= 0).all()                                  # or the voxel would reach the face x = 0
        m = mat[x, p[:, 1], p[:, 2]]
    else:
        m = np.full(len(p), int(material) + 1)
    out = np.concatenate([p, m[:, None]], 1).astype(np.int32)
    if regions is not None:
        regions = [regions] if isinstance(regions, rt.Region) else list(regions)
        out = out[inside(out[:, :3], regions)] if len(regions) else out[:0]
    return _sorted(out)


def filled(V, depth, connectivity=6, material=None, regions=None, fast=False):
    """V + E(V, c) within the mask: what tdt_octree_fill_enclosed leaves, what the solid mesh forms return for V = the surface."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    return _sorted(np.concatenate([V, enclosed(V, depth, connectivity, material, regions, fast=fast)]))


def keys(xyz):
    return _keys(xyz)
