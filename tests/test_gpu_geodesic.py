"""Geodesic distance on the GPU (tdt_octree_geodesic_field / tdt_octree_extract_geodesic / tdt_octree_edit_geodesic /
tdt_octree_geodesic_path): fields, lists and paths must equal the numpy model (tests/geodesic_model.py) element for element, and
the edit form must leave in the bound cells buffer exactly what tdt_octree_edit_voxels of the model's list leaves.  Every
comparison is exact equality, and every case first shows with the model alone that it is what it claims."""
import ctypes
import itertools
import re
import subprocess

import numpy as np
import pytest

import geodesic_model as gm
import tree_model
from test_gpu_connect import bind_tree
from test_gpu_distance import random_tree
from test_gpu_region_edit import apply_op, bind_cells, built_cells, padded, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
OPS = (rt.REGION_SET, rt.REGION_FILL, rt.REGION_PAINT, rt.REGION_CLEAR)
WEIGHTS = ((1, 0, 0), (1, 1, 1), (3, 4, 5), (2, 3, 0), (5, 1, 1), (7, 0, 2))
EDGES = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 62, 63)
BIG = 1 << 30
E, S = rt.MEDIUM_EMPTY, rt.MEDIUM_SOLID


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def same(got, want, tag=""):
    assert got.shape == want.shape and np.array_equal(got, want), tag


def whole(depth):
    n = 1 << depth
    return (0, 0, 0), (n - 1, n - 1, n - 1)


def check_edit(ctx, V, depth, op, lst, tag, **kw):
    """octree_edit_geodesic on a fresh tree of V: the bytes tdt_octree_edit_voxels(op, the model's list) leaves, which are the
    builder's tree of op(V, list)."""
    want = apply_op(V, op, lst, 0)
    built = built_cells(ctx, want, depth, model=len(want) <= 1 << 16)
    have = len(built_cells(ctx, V, depth, model=False)) // 16
    room = max(len(built) // 16 - have, 0) + 8
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    n = ctx.octree_edit_geodesic(op, **kw)
    got = vbo.read(np.uint32)
    assert n == len(built) // 16 and int(counter.read(np.uint32)[0]) == n, tag
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    assert ctx.octree_edit_voxels(op, lst) == n, tag
    assert np.array_equal(got, vbo.read(np.uint32)) and np.array_equal(got, padded(built, got.nbytes)), tag


def check_query(ctx, V, depth, seeds, boxes=(), material=None, edit_op=None, **kw):
    """One query on the bound tree of V against the model: the field over the whole grid and over `boxes`, the list with the
    voxel's own material (SOLID) and an overriding one, optionally the edit form.  Returns the model's g."""
    P, g = gm.solve(V, depth, seeds, **kw)
    for lo, hi in (whole(depth),) + tuple(boxes):
        same(ctx.octree_geodesic_field(seeds, lo, hi, **kw), gm.field(V, depth, seeds, lo, hi, g=g), (kw, lo, hi))
    if kw.get("medium", S) == S:
        same(ctx.octree_extract_geodesic(seeds, **kw), gm.reach_list(V, depth, seeds, g=g), kw)
    lst = gm.reach_list(V, depth, seeds, material=41 if material is None else material, g=g)
    same(ctx.octree_extract_geodesic(seeds, material=41 if material is None else material, **kw), lst, kw)
    if edit_op is not None:
        check_edit(ctx, V, depth, edit_op, lst, (kw, edit_op), seeds=seeds, material=41 if material is None else material, **kw)
        bind_tree(ctx, V, depth)
    return g


# ---- 1. random trees -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("depth", [3, 4, 5, 6])
def test_random_trees_equal_the_model(ctx, depth, w):
    n = 1 << depth
    V = random_tree(depth)
    assert 0 < len(V) < n ** 3
    mat = gm.grid_of(V, depth)
    rng = np.random.default_rng(depth)
    solid_seeds = np.concatenate([V[rng.integers(0, len(V), 3), :3], [[-1, 0, 0], [n, 1, 1]]])
    empties = np.argwhere(mat == 0)
    empty_seeds = np.concatenate([empties[rng.integers(0, len(empties), 3)], [[0, -5, 0]], V[:1, :3]])
    one = int(V[len(V) // 2, 3]) - 1
    mask = [rt.box((1, 0, 2), (n // 2 + 2, n - 2, n - 1)), rt.sphere((n // 2, n // 2, n // 3), n // 3)]
    vbo, counter, _ = bind_tree(ctx, V, depth)
    before = vbo.read(np.uint32)
    cut = 7 * min(v for v in w if v)
    cases = [dict(medium=S, steps=w, max_cost=BIG), dict(medium=E, steps=w, max_cost=cut), dict(medium=S, steps=w, max_cost=BIG, match=one, regions=mask),
             dict(medium=E, steps=w, max_cost=BIG, regions=mask), dict(medium=S, steps=w, max_cost=7), dict(medium=E, steps=w, max_cost=1),
             dict(medium=S, steps=w, max_cost=0), dict(medium=S, steps=w, max_cost=cut, match=one)]
    reach = []
    for i, kw in enumerate(cases):
        seeds = solid_seeds if kw["medium"] == S else empty_seeds
        if kw.get("match") is not None:
            seeds = np.concatenate([seeds, V[V[:, 3] == one + 1][:2, :3]])
        D = gm.domain_box(V, depth, seeds, **kw)
        boxes = ()
        if D is not None and depth > 3:                         # off-centre, and sticking out of D unless D is the whole grid
            lo = tuple(max(D[0][a] - 2, 0) for a in range(3))
            boxes = ((lo, tuple(min(lo[a] + (5, 9, 7)[a], n - 1) for a in range(3))),)
        g = check_query(ctx, V, depth, seeds, boxes, edit_op=OPS[i] if i < 4 else None, **kw)
        reach.append(int((g >= 0).sum()))
    assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345
    # by the model alone: max_cost cuts the reach, a lone seed is all max_cost 0 reaches, and 26-steps reach what 6-steps do not
    assert 0 < reach[6] <= 3 < reach[0] and reach[4] <= reach[0] and reach[5] <= reach[1] and reach[7] > 0
    if depth >= 5:
        assert reach[4] < reach[0] and reach[1] < len(empties)
    if w == (1, 0, 0):
        g6 = gm.solve(V, depth, solid_seeds, steps=(1, 0, 0))[1]
        g26 = gm.solve(V, depth, solid_seeds, steps=(1, 1, 1))[1]
        assert not np.array_equal(g6, g26) and (g26 >= 0).sum() >= (g6 >= 0).sum()


# ---- 2. word, tile and halo boundaries -----------------------------------------------------------------------------------------
def corridors(depth, axis):
    """One-voxel-wide corridors along `axis`, one through every coordinate of EDGES (below N) on the second axis, staggered on
    the third; every other one starts at 1 instead of 0, so that with a seed at either end the cost ridge falls between two
    voxels (on the word boundary 31 | 32 at depth 6) or on one (32).  Returns (voxels, seeds)."""
    n = 1 << depth
    vox, seeds = [], []
    edges = [e for e in EDGES if e < n]
    for k, c in enumerate(edges):
        d = edges[(5 * k + 3) % len(edges)]
        start = k & 1
        for t in range(start, n):
            p = [0, 0, 0]
            p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = t, c, d
            vox.append([*p, 1 + k])
        for t in (start, n - 1):
            p = [0, 0, 0]
            p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = t, c, d
            seeds.append(p)
    vox = np.unique(np.array(vox, np.int32), axis=0)
    _, first = np.unique(vox[:, :3], axis=0, return_index=True)
    return sort_vox(vox[first]), np.array(seeds, np.int32)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("depth,medium", [(6, S), (5, E)])
def test_corridors_across_word_tile_and_halo_boundaries(ctx, depth, medium, axis):
    n = 1 << depth
    C, seeds = corridors(depth, axis)
    if medium == E:                                             # the corridors carved out of a solid grid
        solid = np.ones((n, n, n), bool)
        solid[C[:, 0], C[:, 1], C[:, 2]] = False
        p = np.argwhere(solid)
        V = sort_vox(np.concatenate([p, 1 + (p[:, :1] + p[:, 1:2]) % 7], 1))
    else:
        V = C
    bind_tree(ctx, V, depth)
    for w in ((1, 0, 0), (3, 4, 5)):
        g = check_query(ctx, V, depth, seeds, medium=medium, steps=w, max_cost=BIG)
        line = [0, 0, 0]
        line[(axis + 1) % 3], line[(axis + 2) % 3] = int(C[0, (axis + 1) % 3]), int(C[0, (axis + 2) % 3])
        assert (g >= 0).sum() == len(C) and g.max() >= w[0] * (n // 2 - 1)   # every corridor is walked from both ends to a ridge
        ridge = np.argwhere(g == g.max())
        assert len(ridge) >= 1 and set(ridge[:, axis]) <= {n // 2 - 1, n // 2}


def test_seeds_on_all_eight_grid_corners(ctx):
    depth, n = 5, 32
    V = random_tree(depth)
    mat = gm.grid_of(V, depth)
    seeds = np.array(list(itertools.product((0, n - 1), repeat=3)), np.int32)
    assert sum(int(mat[tuple(s)] == 0) for s in seeds) >= 2
    bind_tree(ctx, V, depth)
    for w in ((1, 1, 1), (3, 4, 5)):
        g = check_query(ctx, V, depth, seeds, medium=E, steps=w, max_cost=BIG)
        assert (g >= 0).sum() > n
    full = sort_vox(np.concatenate([np.argwhere(np.ones((n, n, n), bool)), np.full((n ** 3, 1), 3)], 1))
    bind_tree(ctx, full, depth)
    g = check_query(ctx, full, depth, seeds, medium=S, steps=(1, 0, 0), max_cost=BIG)
    assert g.max() == 3 * (n // 2 - 1) and (g >= 0).all()         # the centre cells: ties between all eight seeds


# ---- 3. many passes ------------------------------------------------------------------------------------------------------------
def serpentine(order, n=32):
    """A one-voxel-wide corridor: runs of 30 along axis order[0], stepping by 2 along order[1], in the plane order[2] = 9.
    Returns (voxels in walking order as (k, 3), the Morton-sorted list)."""
    a, b, c = order
    walk = []
    for i in range(16):
        run = range(1, 31) if i % 2 == 0 else range(30, 0, -1)
        for t in run:
            p = [0, 0, 0]
            p[a], p[b], p[c] = t, 2 * i, 9
            walk.append(p)
        if i < 15:
            p = [0, 0, 0]
            p[a], p[b], p[c] = walk[-1][a], 2 * i + 1, 9
            walk.append(p)
    walk = np.array(walk, np.int32)
    return walk, sort_vox(np.concatenate([walk, 1 + (np.arange(len(walk))[:, None] % 200)], 1))


def test_serpentine_needs_many_passes(ctx):
    passes = {}
    for order in itertools.permutations(range(3)):
        walk, V = serpentine(order)
        assert 480 <= len(walk) <= 520 and len(np.unique(walk, axis=0)) == len(walk)
        bind_tree(ctx, V, 5)
        g = check_query(ctx, V, 5, walk[:1], medium=S, steps=(1, 0, 0), max_cost=BIG)
        assert np.array_equal(g[walk[:, 0], walk[:, 1], walk[:, 2]], np.arange(len(walk)))   # the corridor is walked end to end
        ctx.octree_geodesic_field(walk[:1], *whole(5), medium=S, steps=(1, 0, 0), max_cost=BIG)
        passes[order] = ctx.geodesic_passes()
        g = check_query(ctx, V, 5, walk[:1], medium=S, steps=(1, 0, 0), max_cost=250)
        assert (g >= 0).sum() == 251                             # max_cost ends mid-corridor
        pts, cost = ctx.octree_geodesic_path(walk[:1], walk[-1], medium=S, steps=(1, 0, 0))
        same(pts, walk[::-1].copy(), order)
        assert cost == len(walk) - 1
        pts, cost = ctx.octree_geodesic_path(walk[:1], walk[-1], medium=S, steps=(1, 0, 0), max_cost=250)
        assert len(pts) == 0 and cost == -1
    assert max(passes.values()) > 16, passes                     # more than two batches of passes: the path re-enters tiles


# ---- 4. walls ------------------------------------------------------------------------------------------------------------------
def test_walls_holes_gaps_and_masks(ctx):
    depth, n = 4, 16
    wall = np.array([[8, y, z, 5] for y in range(n) for z in range(n) if (y, z) != (13, 2)], np.int32)
    V = sort_vox(wall)
    bind_tree(ctx, V, depth)
    seed = np.array([[6, 3, 12]], np.int32)
    for w in ((1, 0, 0), (3, 4, 5)):
        g = check_query(ctx, V, depth, seed, medium=E, steps=w, max_cost=BIG)
        free = gm.solve(V[:0], depth, seed, medium=E, steps=w)[1]
        assert g[10, 3, 12] > free[10, 3, 12] and g[8, 13, 2] == free[8, 13, 2] and g[8, 3, 12] == -1   # through the hole, not the wall
    # a diagonal gap: two slabs that share edges only
    slabs = sort_vox(np.array([[x, y, z, 1 + x] for x in range(3, 6) for y in range(2, 9) for z in range(4, 7)] +
                              [[x, y, z, 9] for x in range(6, 9) for y in range(2, 9) for z in range(7, 10)], np.int32))
    bind_tree(ctx, slabs, depth)
    g6 = check_query(ctx, slabs, depth, [(3, 2, 4)], medium=S, steps=(1, 0, 0), max_cost=BIG)
    g26 = check_query(ctx, slabs, depth, [(3, 2, 4)], medium=S, steps=(1, 1, 1), max_cost=BIG)
    assert g6[7, 5, 8] == -1 and g26[7, 5, 8] > 0 and (g6 >= 0).sum() == 63 and (g26 >= 0).sum() == 126
    # a mask that cuts the direct corridor and forces the detour
    block = sort_vox(np.array([[x, y, 5, 2] for x in range(1, 15) for y in range(1, 15)], np.int32))
    bind_tree(ctx, block, depth)
    mask = [rt.box((1, 1, 5), (2, 14, 5)), rt.box((1, 13, 5), (14, 14, 5)), rt.box((13, 1, 5), (14, 14, 5))]      # a U around the middle
    for w in ((1, 0, 0), (1, 1, 1), (3, 4, 5)):
        direct = check_query(ctx, block, depth, [(1, 1, 5)], medium=S, steps=w, max_cost=BIG)
        around = check_query(ctx, block, depth, [(1, 1, 5)], medium=S, steps=w, max_cost=BIG, regions=mask)
        assert around[14, 1, 5] > direct[14, 1, 5] > 0 and around[7, 7, 5] == -1
    # diagonals cheaper than faces: the path to a face neighbour zig-zags through a corner and an edge step
    room = sort_vox(np.array([[x, y, z, 7] for x in range(4, 12) for y in range(4, 12) for z in range(4, 12)], np.int32))
    bind_tree(ctx, room, depth)
    g = check_query(ctx, room, depth, [(7, 7, 7)], medium=S, steps=(5, 1, 1), max_cost=BIG)
    assert g[8, 7, 7] == 2 and g[9, 7, 7] == 2
    pts, cost = ctx.octree_geodesic_path([(7, 7, 7)], (8, 7, 7), medium=S, steps=(5, 1, 1))
    want, wc = gm.path(room, depth, [(7, 7, 7)], (8, 7, 7), steps=(5, 1, 1))
    same(pts, want)
    assert cost == wc == 2 and len(pts) == 3


# ---- 5. paths ------------------------------------------------------------------------------------------------------------------
def test_canonical_paths(ctx):
    depth, n = 5, 32
    room = sort_vox(np.array([[x, y, z, 1 + (x + y) % 5] for x in range(2, 30) for y in range(3, 29) for z in range(10, 16)], np.int32))
    bind_tree(ctx, room, depth)
    two = np.array([[4, 16, 12], [24, 16, 12]], np.int32)         # (14, 16, 12) is 10 from both
    for w in WEIGHTS:
        g = gm.solve(room, depth, two, steps=w)[1]
        assert g[14, 16, 12] == gm.solve(room, depth, two[:1], steps=w)[1][14, 16, 12] == gm.solve(room, depth, two[1:], steps=w)[1][14, 16, 12]
        for goal in ((14, 16, 12), (29, 28, 15), (2, 3, 10), (14, 27, 11)):
            want, wc = gm.path(room, depth, two, goal, steps=w, g=g)
            pts, cost = ctx.octree_geodesic_path(two, goal, medium=S, steps=w)
            same(pts, want, (w, goal))
            assert cost == wc == g[goal] and len(want) >= 2
    # many ties: with 6-steps every monotone staircase is shortest, the canonical one takes -x first, then -y, then -z
    pts, cost = ctx.octree_geodesic_path(two[:1], (9, 20, 14), medium=S, steps=(1, 0, 0))
    assert cost == 5 + 4 + 2 and pts[:6, 0].tolist() == [9, 8, 7, 6, 5, 4] and pts[-1].tolist() == [4, 16, 12]
    # not reached: off the medium, beyond max_cost, off the grid; a goal on a seed is one point
    for goal, kw in (((0, 0, 0), {}), ((29, 28, 15), dict(max_cost=9)), ((-3, 40, 1), {})):
        pts, cost = ctx.octree_geodesic_path(two, goal, medium=S, steps=(1, 1, 1), **kw)
        assert len(pts) == 0 and cost == -1 and gm.path(room, depth, two, goal, steps=(1, 1, 1), **kw)[1] == -1
    pts, cost = ctx.octree_geodesic_path(two, two[1], medium=S, steps=(3, 4, 5))
    assert pts.tolist() == [two[1].tolist()] and cost == 0
    # count-only, and the short capacity: the count, nothing written
    L = rt.lib()
    q = rt.Geodesic(S, -1, (ctypes.c_int32 * 3)(1, 0, 0), BIG, -1, 0)
    goal = (ctypes.c_int32 * 3)(9, 20, 14)
    npts, c = ctypes.c_size_t(0), ctypes.c_int32(0)
    seeds = np.ascontiguousarray(two[:1])
    assert L.tdt_octree_geodesic_path(ctx.h, ctypes.byref(q), seeds.ctypes.data, 1, None, 0, goal, None, 0, ctypes.byref(npts), ctypes.byref(c)) == rt.OK
    assert npts.value == 12 and c.value == 11
    out = np.full((12, 3), 777, np.int32)
    npts = ctypes.c_size_t(0)
    assert L.tdt_octree_geodesic_path(ctx.h, ctypes.byref(q), seeds.ctypes.data, 1, None, 0, goal, out.ctypes.data, 11, ctypes.byref(npts),
                                      ctypes.byref(c)) == rt.ERR_INVALID_VALUE
    assert npts.value == 12 and (out == 777).all()


# ---- 6. the two neighbouring units ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [4, 6])
def test_solid_reach_is_extract_connected(ctx, depth):
    V = random_tree(depth)
    bind_tree(ctx, V, depth)
    seeds = V[[0, len(V) // 3, len(V) - 1], :3]
    for conn, w in ((6, rt.STEPS_6), (26, rt.STEPS_26)):
        got = ctx.octree_extract_geodesic(seeds, medium=S, steps=w)
        same(got, ctx.octree_extract_connected(seeds=seeds, connectivity=conn), conn)
        assert 0 < len(got) <= len(V)
        one = int(V[0, 3]) - 1
        same(ctx.octree_extract_geodesic(seeds[:1], medium=S, steps=w, match=one),
             ctx.octree_extract_connected(seeds=seeds[:1], connectivity=conn, match=rt.MATCH_MATERIAL), (conn, "material"))


@pytest.mark.parametrize("leak", [False, True])
def test_empty_reach_from_the_faces_is_the_complement_of_enclosed(ctx, leak):
    depth, n = 5, 32
    shell = np.array([[x, y, z, 4] for x in range(6, 20) for y in range(8, 25) for z in range(5, 17)
                      if x in (6, 19) or y in (8, 24) or z in (5, 16)], np.int32)
    if leak:
        shell = shell[~((shell[:, 0] == 19) & (shell[:, 1] == 12) & (shell[:, 2] == 9))]
    V = sort_vox(np.concatenate([shell, [[25, 25, 25, 9]]]))
    bind_tree(ctx, V, depth)
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    faces = g[((g == 0) | (g == n - 1)).any(1)]
    empties = n ** 3 - len(V)
    for conn, w in ((6, rt.STEPS_6), (26, rt.STEPS_26)):
        reach = ctx.octree_extract_geodesic(faces, medium=E, steps=w, material=0)
        enclosed = ctx.octree_extract_enclosed(conn, material=0)
        assert len(enclosed) == (0 if leak else 12 * 15 * 10) and len(reach) + len(enclosed) == empties
        both = sort_vox(np.concatenate([reach, enclosed]))
        assert len(np.unique(both[:, :3], axis=0)) == empties    # disjoint, and together every empty voxel


# ---- 7. empties and errors -----------------------------------------------------------------------------------------------------
def test_valid_empty_results(ctx):
    depth, n = 4, 16
    none = np.zeros((0, 4), np.int32)
    vbo, counter, _ = bind_tree(ctx, none, depth, 4)
    assert len(ctx.octree_extract_geodesic([(3, 3, 3)], medium=S)) == 0
    assert (ctx.octree_geodesic_field([(3, 3, 3)], *whole(depth), medium=S) == -1).all()
    assert ctx.octree_geodesic_path([(3, 3, 3)], (3, 3, 3), medium=S) [1] == -1
    assert ctx.octree_edit_geodesic(rt.REGION_CLEAR, [(3, 3, 3)], medium=S) == 1 and not vbo.read(np.uint32).any()
    vbo, counter, _ = bind_tree(ctx, none, depth, 4)
    g = check_query(ctx, none, depth, [(3, 3, 3)], medium=E, steps=(3, 4, 5), max_cost=9)
    assert (g >= 0).sum() > 27
    V = random_tree(depth)
    bind_tree(ctx, V, depth)
    mat = gm.grid_of(V, depth)
    off = np.argwhere(mat == 0)[:3]
    for seeds, kw in (([], dict(medium=S)), ([], dict(medium=E)), (off, dict(medium=S)), (V[:3, :3], dict(medium=E)), ([(-1, 0, 0), (0, n, 0)], dict(medium=S)),
                      (V[:3, :3], dict(medium=S, regions=[])), (V[:3, :3], dict(medium=S, regions=[rt.box((40, 40, 40), (50, 50, 50))]))):
        assert len(ctx.octree_extract_geodesic(seeds, material=3, **kw)) == 0, kw
        assert (ctx.octree_geodesic_field(seeds, *whole(depth), **kw) == -1).all(), kw
        assert ctx.octree_geodesic_path(seeds, V[0, :3], **kw)[1] == -1
    same(ctx.octree_extract_geodesic(V[:3, :3], medium=S, max_cost=0), V[:3])


def test_errors_write_nothing(ctx):
    L = rt.lib()
    depth = 5
    V = random_tree(depth)
    nc, nv, cost = ctypes.c_uint32(0), ctypes.c_size_t(0), ctypes.c_int32(0)
    ok = rt.Geodesic(S, -1, (ctypes.c_int32 * 3)(1, 0, 0), 5, -1, 0)
    lo3, hi3 = (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(3, 3, 3)
    one = np.array([[1, 2, 3]], np.int32)
    fresh = rt.Context(0)
    try:
        for bound in ((), (0,), (7,)):
            for s in bound:
                v = rt.VertexBufferObject(fresh, np.zeros(16, np.uint32) if s == 0 else np.array([depth, 64, 32], np.int32))
                fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, v)
            assert L.tdt_octree_edit_geodesic(fresh.h, 0, ctypes.byref(ok), one.ctypes.data, 1, None, 0, ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract_geodesic(fresh.h, ctypes.byref(ok), one.ctypes.data, 1, None, 0, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_geodesic_field(fresh.h, ctypes.byref(ok), one.ctypes.data, 1, None, 0, lo3, hi3, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_geodesic_path(fresh.h, ctypes.byref(ok), one.ctypes.data, 1, None, 0, lo3, None, 0, ctypes.byref(nv),
                                              ctypes.byref(cost)) == rt.ERR_INCOMPLETE
            fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
    finally:
        fresh.close()
    vbo, counter, _ = bind_tree(ctx, V, depth, 16)
    cells = vbo.read(np.uint32)
    path_before = L.tdt_debug_last_edit_path(ctx.h)

    def unchanged():
        return (np.array_equal(vbo.read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 12345 and
                L.tdt_debug_last_edit_path(ctx.h) == path_before)

    bad_shape = rt.box((0, 0, 0), (1, 1, 1))
    bad_shape.shape = 7
    sd = V[:2, :3]
    X, Ed, F, Pa = ctx.octree_extract_geodesic, ctx.octree_edit_geodesic, ctx.octree_geodesic_field, ctx.octree_geodesic_path
    bad = [dict(medium=2), dict(medium=-1), dict(match=254), dict(match=-2), dict(medium=E, match=3, material=1), dict(steps=(0, 1, 1)),
           dict(steps=(256, 0, 0)), dict(steps=(1, -1, 0)), dict(steps=(1, 0, 256)), dict(max_cost=-1), dict(max_cost=BIG + 1), dict(material=254),
           dict(material=-2), dict(regions=bad_shape), dict(regions=rt.sphere((1, 1, 1), -1))]
    calls = []
    for kw in bad:
        calls += [lambda kw=kw: X(sd, **kw), lambda kw=kw: Ed(rt.REGION_FILL, sd, **kw)]
        rest = {k: v for k, v in kw.items() if k != "material"}
        if rest:
            calls += [lambda rest=rest: F(sd, (0, 0, 0), (3, 3, 3), **rest), lambda rest=rest: Pa(sd, (1, 1, 1), **rest)]
    calls += [lambda: X(sd, medium=E), lambda: Ed(rt.REGION_FILL, sd, medium=E),          # an EMPTY voxel has no material of its own
              lambda: Ed(4, sd), lambda: Ed(-1, sd),
              lambda: F(sd, (-1, 0, 0), (3, 3, 3)), lambda: F(sd, (0, 0, 0), (3, 32, 3)), lambda: F(sd, (0, 4, 0), (3, 3, 3))]
    for i, f in enumerate(calls):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE and unchanged(), i
    padq = rt.Geodesic(S, -1, (ctypes.c_int32 * 3)(1, 0, 0), 5, -1, 1)
    sp = one.ctypes.data
    for rc in (L.tdt_octree_extract_geodesic(ctx.h, None, sp, 1, None, 0, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_geodesic(ctx.h, ctypes.byref(padq), sp, 1, None, 0, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_geodesic(ctx.h, ctypes.byref(ok), None, 1, None, 0, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_geodesic(ctx.h, ctypes.byref(ok), sp, 1, None, 2, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_geodesic(ctx.h, ctypes.byref(ok), sp, 1, None, 0, None, 0, None),
               L.tdt_octree_edit_geodesic(ctx.h, 0, None, sp, 1, None, 0, ctypes.byref(nc)),
               L.tdt_octree_edit_geodesic(ctx.h, 0, ctypes.byref(padq), sp, 1, None, 0, ctypes.byref(nc)),
               L.tdt_octree_edit_geodesic(ctx.h, 0, ctypes.byref(ok), None, 3, None, 0, ctypes.byref(nc)),
               L.tdt_octree_geodesic_field(ctx.h, None, sp, 1, None, 0, lo3, hi3, None, 0, ctypes.byref(nv)),
               L.tdt_octree_geodesic_field(ctx.h, ctypes.byref(ok), sp, 1, None, 0, None, hi3, None, 0, ctypes.byref(nv)),
               L.tdt_octree_geodesic_field(ctx.h, ctypes.byref(ok), sp, 1, None, 0, lo3, None, None, 0, ctypes.byref(nv)),
               L.tdt_octree_geodesic_field(ctx.h, ctypes.byref(ok), sp, 1, None, 0, lo3, hi3, None, 0, None),
               L.tdt_octree_geodesic_path(ctx.h, None, sp, 1, None, 0, lo3, None, 0, ctypes.byref(nv), ctypes.byref(cost)),
               L.tdt_octree_geodesic_path(ctx.h, ctypes.byref(ok), sp, 1, None, 0, None, None, 0, ctypes.byref(nv), ctypes.byref(cost)),
               L.tdt_octree_geodesic_path(ctx.h, ctypes.byref(ok), sp, 1, None, 0, lo3, None, 0, None, ctypes.byref(cost)),
               L.tdt_octree_geodesic_path(ctx.h, ctypes.byref(ok), sp, 1, None, 0, lo3, None, 0, ctypes.byref(nv), None)):
        assert rc == rt.ERR_INVALID_VALUE and unchanged()
    # the list and field forms' short capacity: the count, nothing written
    sd = V[len(V) // 2: len(V) // 2 + 2, :3]
    want = gm.reach_list(V, depth, sd, steps=(1, 1, 1), max_cost=4)
    assert len(want) > 8
    q = rt.Geodesic(S, -1, (ctypes.c_int32 * 3)(1, 1, 1), 4, -1, 0)
    sds = np.ascontiguousarray(sd, np.int32)
    out = np.zeros((len(want), 4), np.int32)
    assert L.tdt_octree_extract_geodesic(ctx.h, ctypes.byref(q), sds.ctypes.data, 2, None, 0, out.ctypes.data, len(want) - 1,
                                         ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
    assert nv.value == len(want) and not out.any()
    f = np.full(64, 777, np.int32)
    assert L.tdt_octree_geodesic_field(ctx.h, ctypes.byref(q), sds.ctypes.data, 2, None, 0, lo3, hi3, f.ctypes.data, 63, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
    assert nv.value == 64 and (f == 777).all() and unchanged()
    assert L.tdt_octree_geodesic_field(ctx.h, ctypes.byref(q), sds.ctypes.data, 2, None, 0, lo3, hi3, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == 64
    # a LEAF value >= 254 cannot be listed: every form refuses it
    badc = cells.copy()
    leaf = np.flatnonzero((badc[1::2] == 2) & (badc[0::2] < 254))[0]
    badc[2 * int(leaf)] = 254
    vbo2, counter2 = bind_cells(ctx, badc, len(badc) // 16)
    for f in (lambda: X(sd), lambda: Ed(rt.REGION_CLEAR, sd), lambda: F(sd, (0, 0, 0), (3, 3, 3)), lambda: Pa(sd, (1, 1, 1))):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE
        assert np.array_equal(vbo2.read(np.uint32), badc) and int(counter2.read(np.uint32)[0]) == 12345
    # a FILL that does not fit: the cell count it needs, nothing written; the same call on a buffer of that size succeeds
    vbo3, counter3, V1 = bind_tree(ctx, np.array([[32, 32, 32, 5]], np.int32), 6)
    chain = vbo3.read(np.uint32)
    kw = dict(medium=E, steps=(1, 1, 1), max_cost=3, material=8)
    lst = gm.reach_list(V1, 6, [(30, 30, 30)], **kw)
    built = built_cells(ctx, apply_op(V1, rt.REGION_FILL, lst, 0), 6)
    need = len(built) // 16
    assert need > len(chain) // 16 and len(lst) == 7 ** 3 - 2     # the cube of three steps, less the voxel and the corner behind it
    with pytest.raises(rt.TdtError) as e:
        Ed(rt.REGION_FILL, [(30, 30, 30)], **kw)
    assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
    assert np.array_equal(vbo3.read(np.uint32), chain) and int(counter3.read(np.uint32)[0]) == 12345
    vbo3, counter3 = bind_cells(ctx, chain, need)
    assert Ed(rt.REGION_FILL, [(30, 30, 30)], **kw) == need
    assert np.array_equal(vbo3.read(np.uint32), built) and int(counter3.read(np.uint32)[0]) == need


def test_domain_cap(ctx):
    """A depth-10 unmasked EMPTY query without a cost limit: the domain is the whole grid, 2^30 voxels, and is refused."""
    depth, n = 10, 1024
    V = sort_vox(np.array([[0, 0, 0, 3], [n - 1, n - 1, n - 1, 8]], np.int32))
    cells = tree_model.build_cells(V, depth)
    vbo, counter = bind_cells(ctx, cells, len(cells) // 16)
    ints = rt.VertexBufferObject(ctx, np.array([depth, 64, n], np.int32))
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
    assert gm.domain_box(V, depth, [(5, 5, 5)], gm.EMPTY, (1, 0, 0), BIG) == ((0, 0, 0), (n - 1, n - 1, n - 1))
    for f in (lambda: ctx.octree_extract_geodesic([(5, 5, 5)], medium=E, material=1), lambda: ctx.octree_geodesic_field([(5, 5, 5)], (0, 0, 0), (3, 3, 3), medium=E),
              lambda: ctx.octree_edit_geodesic(rt.REGION_FILL, [(5, 5, 5)], medium=E, material=1), lambda: ctx.octree_geodesic_path([(5, 5, 5)], (6, 6, 6), medium=E)):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE and "domain" in str(e.value)
    del ints


# ---- a multi-device context ----------------------------------------------------------------------------------------------------
def test_two_share_multi_device_edit_reaches_both_replicas():
    """A two-share context shards the frame over its members, so the frame after the edit shows every replica's cells: it must be,
    bit for bit, the single-device frame after the same edit; the tree, the preview, the field and the path must be the model's."""
    scene = host.Scene.config(2)
    depth = scene.max_depth
    full = sum(8 ** l for l in range(depth))                   # no tree of this depth has more cells: any result fits
    scene.blobs[0] = padded(np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), 64 * full)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    kw = dict(medium=S, steps=rt.CHAMFER_345, max_cost=30)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            V = r.ctx.octree_extract()
            seeds = V[[len(V) // 2], :3]
            preview = r.ctx.octree_extract_geodesic(seeds, **kw)
            n = r.ctx.octree_edit_geodesic(rt.REGION_PAINT, seeds, material=77, **kw)
            n2 = r.ctx.octree_edit_geodesic(rt.REGION_FILL, seeds + [0, 0, 3], medium=E, steps=rt.STEPS_26, max_cost=2, material=5)
            field = r.ctx.octree_geodesic_field(seeds, *whole(depth), **kw)
            pts, cost = r.ctx.octree_geodesic_path(seeds, preview[0, :3], **kw)
            outs.append((n, n2, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), preview, field, pts, np.array([cost])))
            if devices:
                assert rt.lib().tdt_ctx_device_count(r.ctx.h) == 2
        finally:
            r.close()
    one, two = outs
    for k, (a, b) in enumerate(zip(one, two)):                  # counts, cells, frame (by its bits), tree, preview, field, path
        if isinstance(a, np.ndarray) and a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), k
    same(two[5], gm.reach_list(V, depth, seeds, **kw), "preview")
    assert 1 < len(two[5]) < len(V)
    painted = apply_op(V, rt.REGION_PAINT, gm.reach_list(V, depth, seeds, material=77, **kw), 0)
    poured = gm.reach_list(painted, depth, seeds + [0, 0, 3], medium=E, steps=rt.STEPS_26, max_cost=2, material=5)
    want = apply_op(painted, rt.REGION_FILL, poured, 0)
    assert len(poured) > 1 and len(want) == len(V) + len(poured)   # the voxel three above the seed is empty, and air was poured
    same(two[4], want, "the tree after both edits")
    same(two[6], gm.field(want, depth, seeds, *whole(depth), **kw), "field")
    wp, wc = gm.path(want, depth, seeds, two[5][0, :3], **kw)
    same(two[7], wp, "path")
    assert int(two[8][0]) == wc


# ---- the demo ------------------------------------------------------------------------------------------------------------------
def test_demo_reach_click_renders_the_model_tree(tmp_path):
    exe = build.build_demo()
    out = str(tmp_path / "frame.pfm")
    w, h = 96, 64
    scene = host.Scene.config(3)
    depth = scene.max_depth
    cam = host.camera_reference_pose(w, h, 2, 3)
    r = rt.Renderer(scene, cam)
    try:
        xy = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.int32)
        picks = r.pick(xy)
        V = r.ctx.octree_extract()
    finally:
        r.close()
    order = np.argsort(np.abs(xy[:, 0] - w // 2) + np.abs(xy[:, 1] - h // 2), kind="stable")
    px = None
    for i in order:                                              # the pixel nearest the centre with a usable pick
        if picks[i]["status"] == rt.RAY_HIT and picks[i]["fresh_record"]:
            try:
                seed = host.pick_grid_voxel(picks[i], scene, 0)
            except ValueError:
                continue
            px = xy[i]
            break
    assert px is not None, "precondition: a pixel with a hit"
    lst = gm.reach_list(V, depth, [seed], steps=(1, 1, 1), max_cost=6)
    want_vox = apply_op(V, rt.REGION_CLEAR, lst, 0)
    assert 1 < len(lst) < len(V) and len(want_vox) == len(V) - len(lst)
    room = len(np.asarray(scene.blobs[0]).view(np.uint32)) // 16   # the demo uploads the scene's cells buffer as it is
    ctx = rt.Context(0)
    try:
        built = built_cells(ctx, want_vox, depth)
    finally:
        ctx.close()
    n = len(built) // 16
    assert n <= room
    p = subprocess.run([exe, "--config", "3", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "3", "--pick", f"{px[0]},{px[1]}", "--reach", "6",
                        "--steps", "26", "--op", "clear", "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"reach 6 steps 26 medium solid applied cells {n}\b", p.stdout), p.stdout
    fresh = rt.Renderer(host.Scene({**scene.blobs, 0: padded(built, 64 * room)}), cam)
    try:
        ref = fresh.render()
    finally:
        fresh.close()
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF4"
        fw, fh = map(int, f.readline().split())
        f.readline()
        img = np.frombuffer(f.read(), "<f4").reshape(fh, fw, 4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


# ---- 8. depth 7 ----------------------------------------------------------------------------------------------------------------
def test_depth_7_chamfer(ctx):
    """Rows of four words and 16 x 16 tiles of rows: more than one tile along x, more than one batch of tiles."""
    depth, n = 7, 128
    V = random_tree(depth)
    bind_tree(ctx, V, depth)
    seeds = V[[5, len(V) // 2], :3]
    kw = dict(medium=S, steps=rt.CHAMFER_345, max_cost=BIG)
    P, g = gm.solve(V, depth, seeds, **kw)
    assert (g >= 0).sum() > n ** 3 // 8 and g.max() > 3 * n // 2
    same(ctx.octree_geodesic_field(seeds, *whole(depth), **kw), gm.field(V, depth, seeds, *whole(depth), g=g))
    same(ctx.octree_extract_geodesic(seeds, **kw), gm.reach_list(V, depth, seeds, g=g))
    far = tuple(int(v) for v in np.argwhere(g == g.max())[0])
    pts, cost = ctx.octree_geodesic_path(seeds, far, **kw)
    want, wc = gm.path(V, depth, seeds, far, steps=rt.CHAMFER_345, g=g)
    same(pts, want)
    assert cost == wc == g.max()
