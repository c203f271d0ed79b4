"""Voxel smoothing on the GPU (tdt_octree_smooth / tdt_octree_extract_smooth / tdt_octree_density_field): the voxel lists and the
fields must equal the numpy model (tests/smooth_model.py) element for element, inherited materials included, and the edit form
must leave in the bound cells buffer exactly the builder's tree of the model's list.  Every comparison is exact equality."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import distance_model as dm
import smooth_model as sm
from test_gpu_connect import bind_tree, block
from test_gpu_distance import random_tree, tie_pairs
from test_gpu_region_edit import bind_cells, built_cells, padded, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
MODES = (rt.SMOOTH_BOTH, rt.SMOOTH_ADD, rt.SMOOTH_REMOVE)
THRESHOLDS = (0, 1, 20000, 65536)
UNIT = open(os.path.join(build.CSRC, "tdt_smooth.hip")).read()
TILE_Y, TILE_Z = (int(re.search(rf"constexpr int kSmoothTile{a} = (\d+);", UNIT).group(1)) for a in "YZ")


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def same(got, want, tag=""):
    assert got.shape == want.shape and np.array_equal(got, want), tag


def check_edit(ctx, V, depth, want, tag, **kw):
    """octree_smooth on a fresh tree of V: the bytes of the builder's tree of the model's result, the counter set to its cells."""
    built = built_cells(ctx, want, depth, model=len(want) <= 1 << 16)
    have = len(built_cells(ctx, V, depth, model=False)) // 16
    room = max(len(built) // 16 - have, 0) + 8
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    n = ctx.octree_smooth(**kw)
    got = vbo.read(np.uint32)
    assert n == len(built) // 16 and int(counter.read(np.uint32)[0]) == n, tag
    assert np.array_equal(got, padded(built, got.nbytes)), tag


def check_both(ctx, V, depth, tag="", **kw):
    """The extract form and the edit form, each on a fresh tree of V, against the model; returns the model's list."""
    want = sm.smooth(V, depth, **kw)
    bind_tree(ctx, V, depth)
    same(ctx.octree_extract_smooth(**kw), want, (tag, kw))
    check_edit(ctx, V, depth, want, (tag, kw), **kw)
    return want


# ---- 1. random trees -----------------------------------------------------------------------------------------------------------
def cases_of(radius2, n):
    """Every mode, border, threshold, iteration count and material rule, and a box + sphere mask; the long iterations at the radii
    where the model is quick."""
    it = 3 if radius2 <= 16 else 1                               # (the first step's density is shared by all cases: smooth_model keeps it)
    mask = [rt.box((1, 0, 2), (n // 2, n - 2, n - 1)), rt.sphere((n // 2, n // 2, n // 3), n // 3)]
    return [dict(radius2=radius2),
            dict(radius2=radius2, border=1, iterations=it),
            dict(radius2=radius2, threshold=1),
            dict(radius2=radius2, threshold=1, mode=rt.SMOOTH_ADD, material=17, border=1, iterations=it),
            dict(radius2=radius2, threshold=20000, border=1, iterations=it),
            dict(radius2=radius2, threshold=20000, mode=rt.SMOOTH_ADD, material=17, iterations=it),
            dict(radius2=radius2, threshold=20000, mode=rt.SMOOTH_REMOVE, iterations=it),
            dict(radius2=radius2, threshold=65536),
            dict(radius2=radius2, threshold=65536, mode=rt.SMOOTH_REMOVE, border=1),
            dict(radius2=radius2, mode=rt.SMOOTH_REMOVE, iterations=it),
            dict(radius2=radius2, mode=rt.SMOOTH_ADD, border=1, material=0),
            dict(radius2=radius2, regions=mask, border=radius2 % 2, iterations=it),
            dict(radius2=radius2, threshold=20000, mode=rt.SMOOTH_ADD, regions=mask, material=250),
            dict(radius2=radius2, threshold=9000, regions=mask[1], iterations=min(it, 2))]


@pytest.mark.parametrize("radius2", [1, 2, 3, 5, 9, 16, 224, 225])
@pytest.mark.parametrize("depth", [3, 4, 5, 6])
def test_random_trees_equal_the_model(ctx, depth, radius2):
    n = 1 << depth
    V = random_tree(depth)
    assert 0 < len(V) < n ** 3
    bind_tree(ctx, V, depth)
    cases = cases_of(radius2, n)
    wants = [sm.smooth(V, depth, **kw) for kw in cases]
    assert sum(not np.array_equal(want, V) for want in wants) >= 8   # by the model alone: the cases are not fixed points of the tree
    for kw, want in zip(cases, wants):
        same(ctx.octree_extract_smooth(**kw), want, kw)
    same(ctx.octree_extract(), V, "the tree is untouched")
    d, s = ctx.octree_density_field((0, 0, 0), (n - 1, n - 1, n - 1), radius2, support=True)
    wd, ws = sm.field(V, depth, (0, 0, 0), (n - 1, n - 1, n - 1), radius2)
    same(d, wd, "density")
    same(s, ws, "support")
    for kw, want in zip(cases, wants):                          # the edit form of every case
        check_edit(ctx, V, depth, want, kw, **kw)


def test_grid_smaller_than_the_ball(ctx):
    depth, n = 3, 8
    V = random_tree(depth)
    bind_tree(ctx, V, depth)
    assert dm.window_of(225) > n and sm.support(n, 225).max() == n ** 3 < rt.ball_size(225)
    for threshold, mode, border in itertools.product(THRESHOLDS + (3000,), MODES, (0, 1)):
        kw = dict(radius2=225, threshold=threshold, mode=mode, border=border, iterations=2)
        same(ctx.octree_extract_smooth(**kw), sm.smooth(V, depth, **kw), kw)
    check_both(ctx, V, depth, radius2=225, threshold=3000, border=1)
    check_both(ctx, V, depth, radius2=200, threshold=1, material=None)


# ---- 2. word, tile and halo boundaries -----------------------------------------------------------------------------------------
def edge_coordinates(axis, n):
    """x: around the words of a row.  y, z: around the tile's edge, the tile's edge plus the halo of the suite's radii, the far face."""
    if axis == 0:
        return [c for c in (0, 1, 31, 32, 33, 62, 63, 64, 65, n - 1) if c < n]
    t = TILE_Y if axis == 1 else TILE_Z
    c = {0, 1, n - 2, n - 1}
    for k in (1, 2, 3):
        c |= {k * t - 1, k * t, k * t + 1}
    for R in (1, 3, 15):
        c |= {t + R - 1, t + R, 2 * t + R, 2 * t - R - 1 + n // 2}
    return sorted(v for v in c if 0 <= v < n)


def boundary_voxels(depth, axis):
    """A single voxel, a pair or a short bar along `axis` at every edge coordinate (neighbouring coordinates join), each voxel of
    another material, staggered on the two other axes."""
    n = 1 << depth
    out = {}
    for k, c in enumerate(edge_coordinates(axis, n)):
        for j in range(1 + k % 3):                               # one, two or three long
            p = [0, 0, 0]
            p[axis] = min(c + j, n - 1)
            p[(axis + 1) % 3] = (5 + 23 * k) % n
            p[(axis + 2) % 3] = (n - 3 - 37 * k) % n
            out[tuple(p)] = 1 + (10 * k + j) % 254
    return sort_vox(np.array([[*p, m] for p, m in out.items()], np.int32))


@pytest.mark.parametrize("radius2", [1, 9, 225])
@pytest.mark.parametrize("depth,axis", [(7, 0), (6, 1), (6, 2)])
def test_word_tile_and_halo_boundaries(ctx, depth, axis, radius2):
    n = 1 << depth
    V = boundary_voxels(depth, axis)
    assert V[:, axis].min() == 0 and V[:, axis].max() == n - 1  # the domain starts at the grid's face: tiles sit where edge_coordinates aims
    bind_tree(ctx, V, depth)
    want = sm.smooth(V, depth, radius2, threshold=1)
    assert len(set(want[:, 3])) == len(set(V[:, 3])) and len(want) > len(V)
    same(ctx.octree_extract_smooth(radius2, threshold=1), want, "threshold 1, inherited")
    frac = 65536 * 2 // rt.ball_size(radius2)                    # two voxels in the ball pass, one does not: pairs and bars grow, single voxels go
    assert 65536 < frac * rt.ball_size(radius2) <= 2 * 65536
    for border in (0, 1):
        kw = dict(radius2=radius2, threshold=frac, border=border, iterations=2 if radius2 < 225 else 1)
        same(ctx.octree_extract_smooth(**kw), sm.smooth(V, depth, **kw), kw)
    lo, hi = [0, 0, 0], [n - 1, n - 1, n - 1]
    d, s = ctx.octree_density_field(lo, hi, radius2, support=True)
    wd, ws = sm.field(V, depth, lo, hi, radius2)
    same(d, wd, "density")
    same(s, ws, "support")
    lo[(axis + 1) % 3], hi[(axis + 1) % 3] = 3, min(n - 2, 40)  # a slab, unaligned
    same(ctx.octree_density_field(lo, hi, radius2), sm.field(V, depth, lo, hi, radius2)[0], "slab")


def test_the_density_of_one_voxel_is_the_ball(ctx):
    depth, n, c = 6, 64, (40, 20, 23)
    bind_tree(ctx, np.array([[*c, 5]], np.int32), depth)
    d = ctx.octree_density_field((0, 0, 0), (n - 1, n - 1, n - 1), 225)
    ax = np.arange(n)
    ball = ((ax - c[2]) ** 2)[:, None, None] + ((ax - c[1]) ** 2)[None, :, None] + ((ax - c[0]) ** 2)[None, None, :] <= 225
    same(d, ball.astype(np.int32), "the ball itself")
    assert int(d.sum()) == rt.ball_size(225)
    assert int(d[c[2], c[1]].sum()) == 31 == int(d.sum(2).max())  # the widest chord, across the words of the row


# ---- 3. material ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(tie_pairs(6))))
def test_tied_pairs_follow_the_order(ctx, case):
    depth = 6
    pair = np.array(tie_pairs(depth)[case])
    V = sort_vox(np.concatenate([pair, [[5], [200]]], 1))
    assert len(np.unique(V[:, :3], axis=0)) == 2 and dm.sparse_ties(V, depth) > 0
    bind_tree(ctx, V, depth)
    for radius2 in (5, 9, 100):
        want = sm.smooth(V, depth, radius2, threshold=1)
        assert set(want[:, 3]) == {5, 200}
        same(ctx.octree_extract_smooth(radius2, threshold=1), want, radius2)
        same(want, dm.round_op(V, depth, rt.MORPH_DILATE, radius2), "the round unit's rule")


# ---- 4. uniform tiles ----------------------------------------------------------------------------------------------------------
def slab_tree():
    """Depth 7: a solid block three words wide and eight tiles deep against the faces x = 0 and y = 0, far from the others, with a
    noisy +x face and empty space beyond: all-zero tiles, all-ones tiles away from every face, all-ones tiles whose halo leaves the
    grid, and mixed tiles."""
    rng = np.random.default_rng(5)
    solid = np.zeros((128, 128, 128), bool)
    solid[:96, :64, 40:104] = True
    solid[96:101, :64, 40:104] = rng.random((5, 64, 64)) < 0.5
    p = np.argwhere(solid)
    return sort_vox(np.concatenate([p, 1 + (p[:, :1] + 2 * p[:, 1:2] + p[:, 2:3] // 3) % 254], 1))


@pytest.mark.parametrize("radius2", [3, 225])
def test_uniform_tiles(ctx, radius2):
    depth, n = 7, 128
    V = slab_tree()
    R = dm.window_of(radius2)
    occ = dm.grid_of(V, depth) > 0
    # by the model alone: a tile with its halo all ones away from the faces, one all ones against a face, one all zero
    assert occ[:96, 16 - R:24 + R, 56 - R:64 + R].all() and occ[32:64, :8, 56:64].all() and not occ[:, 80:, :].any()
    bind_tree(ctx, V, depth)
    lo, hi = (0, 0, 0), (n - 1, n - 1, n - 1)
    d, s = ctx.octree_density_field(lo, hi, radius2, support=True)
    wd, ws = sm.field(V, depth, lo, hi, radius2)
    assert (wd == rt.ball_size(radius2)).any() and (wd == 0).any() and (ws < rt.ball_size(radius2)).any()
    same(d, wd, "density")
    same(s, ws, "support")
    for border in (0, 1):
        for kw in (dict(radius2=radius2, border=border), dict(radius2=radius2, border=border, threshold=40000, mode=rt.SMOOTH_REMOVE)):
            want = sm.smooth(V, depth, **kw)
            assert 0 < len(want) and not np.array_equal(want, V)
            same(ctx.octree_extract_smooth(**kw), want, kw)
    want = sm.smooth(V, depth, radius2, border=1)
    check_edit(ctx, V, depth, want, "edit", radius2=radius2, border=1)


# ---- 5. against the round unit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [4, 6])
def test_against_the_round_morphology(ctx, depth):
    V = random_tree(depth)
    bind_tree(ctx, V, depth)
    for radius2 in (1, 5, 16, 225):
        for material in (None, 40):
            same(ctx.octree_extract_smooth(radius2, threshold=1, material=material), ctx.octree_extract_morph_round(rt.MORPH_DILATE, radius2, material=material),
                 (radius2, material))
        for border in (0, 1):
            same(ctx.octree_extract_smooth(radius2, threshold=65536, border=border), ctx.octree_extract_morph_round(rt.MORPH_ERODE, radius2, border=border),
                 (radius2, border))


# ---- 6. the field --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius2", [1, 9, 225])
def test_density_field(ctx, radius2):
    depth, n = 5, 32
    V = random_tree(depth)
    vbo, counter, _ = bind_tree(ctx, V, depth)
    before = vbo.read(np.uint32)
    for lo, hi in (((0, 0, 0), (n - 1, n - 1, n - 1)), ((3, 5, 1), (29, 17, 30)), ((7, 0, 0), (7, n - 1, n - 1)), ((0, 13, 2), (n - 1, 13, 2)),
                   ((30, 31, 0), (30, 31, 0)), ((0, 0, 0), (0, 0, 0))):
        wd, ws = sm.field(V, depth, lo, hi, radius2)
        same(ctx.octree_density_field(lo, hi, radius2), wd, (lo, hi))
        d, s = ctx.octree_density_field(lo, hi, radius2, support=True)
        same(d, wd, (lo, hi))
        same(s, ws, (lo, hi))
        assert (d <= s).all() and (s >= 1).all() and (s <= rt.ball_size(radius2)).all()
    assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345
    # the count-only call and the short capacity
    L = rt.lib()
    lo, hi = (ctypes.c_int32 * 3)(1, 2, 3), (ctypes.c_int32 * 3)(4, 4, 4)
    nv = ctypes.c_size_t(0)
    assert L.tdt_octree_density_field(ctx.h, lo, hi, radius2, None, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == 4 * 3 * 2
    out = np.full(24, 777, np.int32)
    nv = ctypes.c_size_t(0)
    assert L.tdt_octree_density_field(ctx.h, lo, hi, radius2, out.ctypes.data, None, 23, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
    assert nv.value == 24 and (out == 777).all()


# ---- 7. empty trees, empty results, fixed points -------------------------------------------------------------------------------
def test_empty_tree_and_a_result_that_becomes_empty(ctx):
    depth = 4
    vbo, counter, _ = bind_tree(ctx, np.zeros((0, 4), np.int32), depth, 4)
    d, s = ctx.octree_density_field((0, 0, 0), (15, 15, 15), 9, support=True)
    assert (d == 0).all()
    same(s, sm.support(16, 9).transpose(2, 1, 0), "the support of the empty tree")
    for mode in MODES:
        assert len(ctx.octree_extract_smooth(4, mode=mode, threshold=1)) == 0
        assert ctx.octree_smooth(4, mode=mode, threshold=1) == 1
        assert not vbo.read(np.uint32).any() and int(counter.read(np.uint32)[0]) == 1
    V = sort_vox(np.array([[3, 4, 5, 9], [12, 1, 0, 77], [13, 1, 0, 78]], np.int32))    # a single voxel and a pair vanish under majority
    vbo, counter, _ = bind_tree(ctx, V, depth, 4)
    assert len(sm.smooth(V, depth, 2)) == 0 and len(ctx.octree_extract_smooth(2)) == 0
    assert ctx.octree_smooth(2, iterations=4) == 1
    assert not vbo.read(np.uint32).any() and int(counter.read(np.uint32)[0]) == 1      # the all-EMPTY root
    bind_tree(ctx, V, depth)
    same(ctx.octree_extract_smooth(2, mode=rt.SMOOTH_ADD), V, "nothing to add")


def test_iterations_past_a_fixed_point(ctx):
    depth, n = 5, 32
    V = random_tree(depth)
    fixed = None
    for k in range(1, 17):                                      # by the model alone: where the majority filter settles
        nxt = sm.smooth(V, depth, 3, iterations=k, border=1)
        if fixed is not None and np.array_equal(nxt, fixed):
            break
        fixed = nxt
    assert 2 <= k <= 12 and len(fixed)
    bind_tree(ctx, V, depth)
    same(ctx.octree_extract_smooth(3, iterations=k - 1, border=1), fixed, "at the fixed point")
    same(ctx.octree_extract_smooth(3, iterations=16, border=1), fixed, "past it")
    check_edit(ctx, V, depth, fixed, "edit", radius2=3, iterations=16, border=1)
    slab = sort_vox(block((0, 0, 0), (n - 1, n - 1, 5), 7))     # a slab cut by five faces: fixed from the start with border 1 only
    bind_tree(ctx, slab, depth)
    same(ctx.octree_extract_smooth(9, iterations=16, border=1), slab, "a fixed point")
    cut = sm.smooth(slab, depth, 9, iterations=2, border=0)
    assert len(cut) < len(slab)
    same(ctx.octree_extract_smooth(9, iterations=2, border=0), cut, "rounded off at the faces")


# ---- 8. errors and limits ------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(ctx):
    L = rt.lib()
    depth = 5
    V = random_tree(depth)
    nc, nv = ctypes.c_uint32(0), ctypes.c_size_t(0)
    ok = rt.Smooth(3, 1, 0, rt.SMOOTH_BOTH, -1, 0)
    lo3, hi3 = (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(3, 3, 3)
    fresh = rt.Context(0)
    try:
        for bound in ((), (0,), (7,)):
            for s in bound:
                v = rt.VertexBufferObject(fresh, np.zeros(16, np.uint32) if s == 0 else np.array([depth, 64, 32], np.int32))
                fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, v)
            assert L.tdt_octree_smooth(fresh.h, ctypes.byref(ok), None, 0, ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract_smooth(fresh.h, ctypes.byref(ok), None, 0, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_density_field(fresh.h, lo3, hi3, 4, None, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
    finally:
        fresh.close()
    vbo, counter, _ = bind_tree(ctx, V, depth, 16)
    cells = vbo.read(np.uint32)

    def unchanged():
        return np.array_equal(vbo.read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 12345

    bad_shape = rt.box((0, 0, 0), (1, 1, 1))
    bad_shape.shape = 7
    M, X, F = ctx.octree_smooth, ctx.octree_extract_smooth, ctx.octree_density_field
    cases = [lambda: M(0), lambda: M(226), lambda: M(-4), lambda: M(3, iterations=0), lambda: M(3, iterations=17), lambda: M(3, threshold=-1),
             lambda: M(3, threshold=65537), lambda: M(3, mode=3), lambda: M(3, mode=-1), lambda: M(3, material=254), lambda: M(3, material=-2),
             lambda: M(3, border=2), lambda: M(3, border=-1), lambda: M(3, regions=bad_shape), lambda: M(3, regions=rt.sphere((1, 1, 1), -1)),
             lambda: X(0), lambda: X(4096), lambda: X(3, iterations=-1), lambda: X(3, threshold=1 << 20), lambda: X(3, mode=7),
             lambda: X(3, material=300), lambda: X(3, border=3), lambda: X(3, regions=bad_shape),
             lambda: F((0, 0, 0), (3, 3, 3), 0), lambda: F((0, 0, 0), (3, 3, 3), 226), lambda: F((-1, 0, 0), (3, 3, 3), 4),
             lambda: F((0, 0, 0), (3, 32, 3), 4), lambda: F((0, 4, 0), (3, 3, 3), 4)]
    for i, f in enumerate(cases):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE and unchanged(), i
    for rc in (L.tdt_octree_smooth(ctx.h, None, None, 0, ctypes.byref(nc)),
               L.tdt_octree_smooth(ctx.h, ctypes.byref(ok), None, 1, ctypes.byref(nc)),
               L.tdt_octree_extract_smooth(ctx.h, ctypes.byref(ok), None, 2, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_smooth(ctx.h, None, None, 0, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_smooth(ctx.h, ctypes.byref(ok), None, 0, None, 0, None),
               L.tdt_octree_density_field(ctx.h, None, hi3, 4, None, None, 0, ctypes.byref(nv)),
               L.tdt_octree_density_field(ctx.h, lo3, None, 4, None, None, 0, ctypes.byref(nv)),
               L.tdt_octree_density_field(ctx.h, lo3, hi3, 4, None, None, 0, None)):
        assert rc == rt.ERR_INVALID_VALUE and unchanged()
    assert nc.value == 0
    # the extract form's short capacity: the count, nothing written
    want = sm.smooth(V, depth, 3)
    out = np.zeros((len(want), 4), np.int32)
    assert L.tdt_octree_extract_smooth(ctx.h, ctypes.byref(ok), None, 0, out.ctypes.data, len(want) - 1, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
    assert nv.value == len(want) and not out.any()
    # a LEAF value >= 254 cannot be rebuilt: every form refuses it
    bad = cells.copy()
    leaf = np.flatnonzero((bad[1::2] == 2) & (bad[0::2] < 254))[0]
    bad[2 * int(leaf)] = 254
    vbo2, counter2 = bind_cells(ctx, bad, len(bad) // 16)
    for f in (lambda: M(3), lambda: X(3), lambda: F((0, 0, 0), (3, 3, 3), 4)):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE
        assert np.array_equal(vbo2.read(np.uint32), bad) and int(counter2.read(np.uint32)[0]) == 12345
    # a growth that does not fit: the cell count it needs, nothing written; the same call on a buffer of that size succeeds
    vbo3, counter3, V1 = bind_tree(ctx, np.array([[32, 32, 32, 5]], np.int32), 6)
    chain = vbo3.read(np.uint32)
    built = built_cells(ctx, sm.smooth(V1, 6, 4, threshold=1), 6)
    need = len(built) // 16
    assert need > len(chain) // 16
    with pytest.raises(rt.TdtError) as e:
        M(4, threshold=1)
    assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
    assert np.array_equal(vbo3.read(np.uint32), chain) and int(counter3.read(np.uint32)[0]) == 12345
    vbo3, counter3 = bind_cells(ctx, chain, need)
    assert M(4, threshold=1) == need
    assert np.array_equal(vbo3.read(np.uint32), built) and int(counter3.read(np.uint32)[0]) == need


def test_domain_cap(ctx):
    """Depth 10, two voxels 600 apart on every axis: the bounding box holds 2.16e8 voxels, under the cap of 2^28, and a majority
    with an empty outside runs on it as it is; a filter that can grow is refused before any volume is allocated, because the box
    grown by iterations * R is the whole grid, 2^30 voxels.  At opposite corners of the grid every form is refused."""
    depth, n = 10, 1024
    V = sort_vox(np.array([[0, 0, 0, 3], [599, 599, 599, 8]], np.int32))
    vbo, counter, _ = bind_tree(ctx, V, depth, 64)
    cells = vbo.read(np.uint32)
    for kw in (dict(radius2=225, iterations=16, threshold=1), dict(radius2=225, iterations=16, border=1), dict(radius2=225, iterations=16, threshold=32768)):
        for f in (ctx.octree_smooth, ctx.octree_extract_smooth):
            with pytest.raises(rt.TdtError) as e:
                f(**kw)
            assert e.value.code == rt.ERR_INVALID_VALUE and "domain" in str(e.value), kw
            assert np.array_equal(vbo.read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 12345
    assert len(ctx.octree_extract_smooth(225, iterations=16)) == 0                  # no growth: the box itself
    same(ctx.octree_extract_smooth(225, iterations=16, threshold=32769, mode=rt.SMOOTH_ADD), V, "no growth above one half")
    V = sort_vox(np.array([[0, 0, 0, 3], [n - 1, n - 1, n - 1, 8]], np.int32))
    bind_tree(ctx, V, depth, 64)
    with pytest.raises(rt.TdtError) as e:
        ctx.octree_extract_smooth(1)
    assert e.value.code == rt.ERR_INVALID_VALUE and "domain" in str(e.value)
    with pytest.raises(rt.TdtError) as e:                        # a field box above 2^26 voxels
        ctx.octree_density_field((0, 0, 0), (n - 1, n - 1, 64), 1)
    assert e.value.code == rt.ERR_INVALID_VALUE


def test_two_share_multi_device_edit_reaches_both_replicas():
    """A two-share context shards the frame over its members, so the frame after the edit shows every replica's cells: it must be,
    bit for bit, the single-device frame after the same edit and the frame of a fresh upload of the model's tree."""
    scene = host.Scene.config(2)
    depth = scene.max_depth
    full = sum(8 ** l for l in range(depth))                   # no tree of this depth has more cells: any result fits
    scene.blobs[0] = padded(np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), 64 * full)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            V = r.ctx.octree_extract()
            c = V[len(V) // 2, :3].astype(int)
            mask = [rt.sphere(c, 12)]
            preview = r.ctx.octree_extract_smooth(5, iterations=2)
            n = r.ctx.octree_smooth(5, iterations=2)
            n2 = r.ctx.octree_smooth(4, threshold=20000, mode=rt.SMOOTH_ADD, regions=mask)
            field = r.ctx.octree_density_field((0, 0, 0), (63, 63, 63), 9)
            outs.append((n, n2, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), preview, field))
            if devices:
                assert rt.lib().tdt_ctx_device_count(r.ctx.h) == 2
        finally:
            r.close()
    one, two = outs
    for k, (a, b) in enumerate(zip(one, two)):                  # counts, cells, frame (by its bits), tree, preview, field
        if isinstance(a, np.ndarray) and a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), k
    smoothed = sm.smooth(V, depth, 5, iterations=2)
    same(two[5], smoothed, "preview")
    want = sm.smooth(smoothed, depth, 4, threshold=20000, mode=rt.SMOOTH_ADD, regions=mask)
    assert not np.array_equal(smoothed, V) and not np.array_equal(want, smoothed)
    same(two[4], want, "the tree after both edits")
    same(two[6], sm.field(want, depth, (0, 0, 0), (63, 63, 63), 9)[0], "field")
    ctx = rt.Context(0)
    try:
        built = built_cells(ctx, want, depth, model=False)
    finally:
        ctx.close()
    assert two[1] == len(built) // 16 and np.array_equal(two[2], padded(built, 64 * full))
    fresh = rt.Renderer(host.Scene({**scene.blobs, 0: padded(built, 64 * full)}), cam)
    try:
        ref = fresh.render()
    finally:
        fresh.close()
    assert (two[3].view(np.uint32) == ref.view(np.uint32)).all()


# ---- 9. the demo ---------------------------------------------------------------------------------------------------------------
def test_demo_smooth_leaves_the_model_tree(tmp_path):
    exe = build.build_demo()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    room = len(np.asarray(scene.blobs[0]).view(np.uint32)) // 16
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        want = sm.smooth(V, depth, 5, iterations=2, threshold=20000, mode=rt.SMOOTH_ADD, material=9, border=1)
        n = len(built_cells(ctx, want, depth)) // 16
        del vbos
    finally:
        ctx.close()
    assert len(want) > len(V)
    p = subprocess.run([exe, "--config", "2", "--size", "64x48", "--spp", "1", "--bounce", "2", "--cells", str(max(room, n)), "--smooth", "5:2",
                        "--threshold", "20000", "--smooth-mode", "add", "--material", "9", "--border", "1", "--out", str(tmp_path / "frame.pfm")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"smooth 5:2 threshold 20000 mode 1 border 1 cells {n}\b", p.stdout), p.stdout
