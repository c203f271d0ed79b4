"""The numpy model of geodesic distance (include/tdt_rt.h tdt_octree_geodesic_field and its siblings), the yardstick of the GPU
tests: the medium P on a dense grid, then a bucketed, Dial-style relaxation — the voxels whose tentative cost is c are settled
together, level by level, and push c + w into their neighbours' buckets — so a 64^3 grid takes seconds.  The whole grid is held,
so it serves depths up to 7; numpy only.  tests/test_geodesic_api.py pins it to a plain heapq Dijkstra."""
import heapq

import numpy as np

from test_gpu_region_edit import inside, sort_vox
from tdt4230_project_raytracing_amd import rt

EMPTY, SOLID = 0, 1
# the 26 offsets in ascending t(d) = 9 (dx + 1) + 3 (dy + 1) + (dz + 1), with their class k(d) = |dx| + |dy| + |dz| - 1
OFFSETS = [((dx, dy, dz), abs(dx) + abs(dy) + abs(dz) - 1) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def grid_of(V, depth):
    """mat[x, y, z] = material + 1 of the voxel there, 0 where the grid is empty."""
    n = 1 << depth
    V = np.asarray(V, np.int64).reshape(-1, 4)
    mat = np.zeros((n, n, n), np.int16)
    mat[V[:, 0], V[:, 1], V[:, 2]] = V[:, 3]
    return mat


def _region_list(regions):
    return None if regions is None else ([regions] if isinstance(regions, rt.Region) else list(regions))


def medium_of(V, depth, medium=SOLID, match=None, regions=None):
    """P as a boolean grid [x, y, z].  regions None: no mask; an empty list: an empty mask."""
    n = 1 << depth
    mat = grid_of(V, depth)
    P = mat == 0 if medium == EMPTY else (mat > 0 if match is None else mat == match + 1)
    regions = _region_list(regions)
    if regions is not None:
        g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
        P = P & (inside(g, regions).reshape(n, n, n) if regions else False)
    return P


def _valid_seeds(P, seeds):
    n = P.shape[0]
    s = np.asarray(seeds, np.int64).reshape(-1, 3)
    s = s[((s >= 0) & (s < n)).all(1)]
    return s[P[s[:, 0], s[:, 1], s[:, 2]]] if len(s) else s


def distances(P, seeds, steps, max_cost=1 << 30):
    """g over the grid as int64 [x, y, z]: the cost for the voxels of R, -1 for every other one."""
    n = P.shape[0]
    w = [int(v) for v in steps]
    assert 1 <= w[0] <= 255 and 0 <= w[1] <= 255 and 0 <= w[2] <= 255
    INF = np.int64(1) << 40
    dist = np.full(n * n * n, INF, np.int64)
    flatP = P.reshape(-1)
    s = _valid_seeds(P, seeds)
    buckets, levels = {}, []
    if len(s):
        start = np.unique((s[:, 0] * n + s[:, 1]) * n + s[:, 2])
        dist[start] = 0
        buckets[0] = [start]
        levels = [0]
    while levels:
        c = heapq.heappop(levels)
        if c > max_cost:
            break
        idx = np.unique(np.concatenate(buckets.pop(c)))
        idx = idx[dist[idx] == c]                               # the others were lowered since they were pushed
        if not len(idx):
            continue
        x, y, z = idx // (n * n), (idx // n) % n, idx % n
        for (dx, dy, dz), k in OFFSETS:
            if not w[k] or c + w[k] > max_cost:
                continue
            qx, qy, qz = x + dx, y + dy, z + dz
            ok = (qx >= 0) & (qx < n) & (qy >= 0) & (qy < n) & (qz >= 0) & (qz < n)
            q = ((qx * n + qy) * n + qz)[ok]
            q = q[flatP[q] & (dist[q] > c + w[k])]
            if len(q):
                dist[q] = c + w[k]
                if c + w[k] not in buckets:
                    buckets[c + w[k]] = []
                    heapq.heappush(levels, c + w[k])
                buckets[c + w[k]].append(q)
    dist[dist > max_cost] = -1
    return dist.reshape(n, n, n)


def solve(V, depth, seeds, medium=SOLID, steps=(1, 0, 0), max_cost=1 << 30, match=None, regions=None):
    """(P, g): the medium and the distances of one query."""
    P = medium_of(V, depth, medium, match, regions)
    return P, distances(P, seeds, steps, max_cost)


def field(V, depth, seeds, lo, hi, g=None, **kw):
    """What tdt_octree_geodesic_field returns over the inclusive box lo..hi: an (ez, ey, ex) int32 array."""
    if g is None:
        g = solve(V, depth, seeds, **kw)[1]
    return np.ascontiguousarray(g[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1].transpose(2, 1, 0).astype(np.int32))


def reach_list(V, depth, seeds, material=None, g=None, **kw):
    """What tdt_octree_extract_geodesic returns: R as {x, y, z, m}, Morton-sorted; material None: the voxel's own."""
    if g is None:
        g = solve(V, depth, seeds, **kw)[1]
    p = np.argwhere(g >= 0)
    mat = grid_of(V, depth)
    m = mat[p[:, 0], p[:, 1], p[:, 2]].astype(np.int64) if material is None else np.full(len(p), int(material) + 1)
    if material is None:
        assert (m > 0).all()                                    # only the SOLID medium has materials of its own
    return sort_vox(np.concatenate([p, m[:, None]], 1))


def path(V, depth, seeds, goal, steps=(1, 0, 0), g=None, **kw):
    """(the canonical shortest path from goal as an (n, 3) int32 array, g(goal)); (an empty array, -1) for a goal not in R.
    (A voxel with g >= 0 is in P, and g(p) + w == g(q) <= max_cost puts p in R: the step's ends need no further test.)"""
    if g is None:
        g = solve(V, depth, seeds, steps=steps, **kw)[1]
    n = g.shape[0]
    q = tuple(int(v) for v in goal)
    if not all(0 <= v < n for v in q) or g[q] < 0:
        return np.zeros((0, 3), np.int32), -1
    out = [q]
    while g[q] > 0:
        for (dx, dy, dz), k in OFFSETS:                         # ascending t(d)
            p = (q[0] + dx, q[1] + dy, q[2] + dz)
            if steps[k] and all(0 <= v < n for v in p) and g[p] >= 0 and g[p] + steps[k] == g[q]:
                q = p
                break
        else:
            raise AssertionError("a voxel of R without a predecessor")
        out.append(q)
    return np.array(out, np.int32), int(g[tuple(int(v) for v in goal)])


def domain_box(V, depth, seeds, medium=SOLID, steps=(1, 0, 0), max_cost=1 << 30, match=None, regions=None):
    """The box D of the header's domain rule as (lo, hi), inclusive, or None when it is empty."""
    n = 1 << depth
    lo, hi = np.zeros(3, np.int64), np.full(3, n - 1, np.int64)
    regions = _region_list(regions)
    if regions is not None:
        mlo, mhi = np.full(3, 1 << 40, np.int64), np.full(3, -(1 << 40), np.int64)
        for r in regions:
            a, b = np.array(list(r.a), np.int64), np.array(list(r.b), np.int64)
            rlo, rhi = (a, b) if r.shape == rt.SHAPE_BOX else (a - b[0], a + b[0])
            if (rlo <= rhi).all():
                mlo, mhi = np.minimum(mlo, rlo), np.maximum(mhi, rhi)
        lo, hi = np.maximum(lo, mlo), np.minimum(hi, mhi)
    V = np.asarray(V, np.int64).reshape(-1, 4)
    if medium == SOLID:
        if not len(V):
            return None
        lo, hi = np.maximum(lo, V[:, :3].min(0)), np.minimum(hi, V[:, :3].max(0))
    s = np.asarray(seeds, np.int64).reshape(-1, 3)
    s = s[((s >= 0) & (s < n)).all(1)]
    if not len(s):
        return None
    grow = int(max_cost) // min(int(v) for v in steps if v > 0)
    lo, hi = np.maximum(lo, s.min(0) - grow), np.minimum(hi, s.max(0) + grow)
    return None if (lo > hi).any() else (tuple(int(v) for v in lo), tuple(int(v) for v in hi))
