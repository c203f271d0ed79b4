"""Stroke brushes (tdt_voxelize_stroke / tdt_octree_edit_stroke / tdt_octree_extract_stroke): the voxel list must equal the numpy
model (tests/stroke_model.py: the header's integer tests, highest segment wins) bit for bit, the edit form must leave in the bound
cells buffer exactly what tdt_octree_edit_voxels of that list leaves — the builder's tree of op(V, list) followed by zeros — and
the extract form must return the tree's voxels the list holds."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import stroke_model as sm
from test_gpu_connect import bind_tree, block
from test_gpu_region_edit import apply_op, bind_cells, built_cells, expected_bytes, padded
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
OPS = (rt.REGION_SET, rt.REGION_FILL, rt.REGION_PAINT, rt.REGION_CLEAR)
NIBS = (rt.SHAPE_SPHERE, rt.SHAPE_BOX)


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def check(ctx, pts, r, depth, segments=None, materials=None, material=0, shape=rt.SHAPE_SPHERE, tag=""):
    want = sm.voxelize(pts, r, depth, segments, materials, material, shape)
    got = ctx.voxelize_stroke(pts, r, depth, segments, materials, material, shape)
    assert got.shape == want.shape and np.array_equal(got, want), (tag, shape, r)
    return want


def check_both(ctx, pts, r, depth, **kw):
    return [check(ctx, pts, r, depth, shape=shape, **kw) for shape in NIBS]


# ---- 1. random strokes of both nibs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 5, 6])
def test_extract_equals_the_model(ctx, depth):
    rng = np.random.default_rng(200 + depth)
    n = 1 << depth
    pts, mats = sm.random_stroke(rng, 48, n)
    # the stroke leaves the grid through all six faces
    pts[3], pts[4] = [-n // 2, 1, 2], [n - 1 + n // 2, n - 2, n - 1]
    pts[9], pts[10] = [2, -n // 2, n - 3], [n - 1, n - 1 + n // 2, 0]
    pts[15], pts[16] = [n // 3, n - 1, -n // 2], [n // 2, 0, n - 1 + n // 2]
    assert (pts.min(0) < 0).all() and (pts.max(0) > n - 1).all()
    for shape in NIBS:
        r = 2 if depth > 3 else 1
        want = check(ctx, pts, r, depth, materials=mats, shape=shape)
        assert len(want) > 0
        for a in range(3):
            assert want[:, a].min() == 0 and want[:, a].max() == n - 1
        # the tie rule is exercised: some voxel is covered by segments of different materials
        per = np.concatenate([sm.voxelize(pts[i:i + 2], r, depth, material=int(mats[i]) - 1, shape=shape) for i in range(len(mats))])
        key = sm.morton(per[:, :3])
        order = np.argsort(key, kind="stable")
        key, m = key[order], per[order, 3]
        assert ((key[1:] == key[:-1]) & (m[1:] != m[:-1])).any()
        # the uniform-material form, and another radius
        check(ctx, pts, r + 3, depth, material=17, shape=shape)


# ---- 2. tile edges -----------------------------------------------------------------------------------------------------------
def test_tile_edges(ctx):
    for depth in (4, 5):
        # inside one tile
        for want in check_both(ctx, [[9, 10, 11], [13, 12, 14]], 0, depth):
            assert len(want) > 0 and (want[:, :3] // 8 == 1).all()
        check_both(ctx, [[10, 10, 10], [12, 13, 11]], 1, depth)
        # along the plane between voxels 7 and 8: on x = 7 and on x = 8, radius 0 and 1 (both sides of the tile border are reached)
        for x in (7, 8):
            check_both(ctx, [[x, 2, 3], [x, 13, 12]], 0, depth)
            for want in check_both(ctx, [[x, 2, 3], [x, 13, 12]], 1, depth):
                assert {7, 8} <= set(want[:, 0])
        # ending exactly on a tile corner
        for want in check_both(ctx, [[8, 8, 8], [3, 5, 1]], 2, depth, material=3):
            assert {(x, y, z) for x in (7, 8) for y in (7, 8) for z in (7, 8)} <= {tuple(p) for p in want[:, :3]} and set(want[:, 3]) == {4}
        check_both(ctx, [[8, 8, 8], [15, 15, 15]], 0, depth)
        # a voxel range of 3 x 5 x 7 (fewer than 64 voxels per step would fill) and one of 9 x 9 x 9 (a ragged last step)
        for want in check_both(ctx, [[1, 1, 1], [1, 3, 5]], 1, depth):
            assert (want[:, :3].max(0) - want[:, :3].min(0) + 1 <= (3, 5, 7)).all()
        ball, box = check_both(ctx, [[4, 4, 4]], 4, depth)
        assert len(box) == 729 and 0 < len(ball) < 729
        check_both(ctx, [[2, 3, 4], [6, 7, 8]], 2, depth)


# ---- 3. the grid's edge, radius 0, the largest radius ---------------------------------------------------------------------------
def test_off_grid_radius_zero_and_the_largest_radius(ctx):
    # wholly off the grid: nothing (before the tiles, in the cull, and in the voxel test)
    for pts, r in (([[-30, -30, -30], [-20, 100, -25]], 3), ([[-9, 5, 5], [-5, 40, 5]], 4), ([[40, -9, -9], [-9, 40, -9]], 6),
                   ([[8192, 8192, 8192], [-8192, 8192, 8192]], 2048)):
        for shape in NIBS:
            assert ctx.voxelize_stroke(pts, r, 5, shape=shape).shape == (0, 4)
            assert sm.voxelize(pts, r, 5, shape=shape).shape == (0, 4)
    # a corner cut off: the round nib's tiles pass the cull and hold no covered voxel (the line is 7.07 away, the radius is 7)
    assert check(ctx, [[-20, 10, 5], [10, -20, 5]], 7, 5).shape == (0, 4)
    assert len(check(ctx, [[-20, 10, 5], [10, -20, 5]], 7, 5, shape=rt.SHAPE_BOX)) > 0
    assert len(check(ctx, [[-20, 10, 5], [10, -20, 5]], 8, 5)) > 0
    # both ends off the grid, only the middle crossing it; the far ends at the coordinate limit
    for pts in ([[-20, 3, -7], [50, 20, 40]], [[-8192, -8192, -8192], [8192, 8192, 8190]], [[8192, -8192, 5], [-8192, 8192, 25]]):
        for want in check_both(ctx, pts, 1, 5):
            assert len(want) > 0
    # radius 0: the lattice points on a body diagonal and on a generic segment
    for shape in NIBS:
        assert check(ctx, [[0, 0, 0], [31, 31, 31]], 0, 5, shape=shape)[:, :3].tolist() == [[i, i, i] for i in range(32)]
        want = check(ctx, [[1, 2, 3], [7, 5, 15]], 0, 5, shape=shape, material=9)
        assert {tuple(p) for p in want} == {(1, 2, 3, 10), (3, 3, 7, 10), (5, 4, 11, 10), (7, 5, 15, 10)}
    # the largest radius at depth 3: every voxel
    for shape in NIBS:
        assert len(check(ctx, [[3, 4, 5]], rt.STROKE_RADIUS_MAX, 3, shape=shape)) == 512
        assert len(check(ctx, [[-8192, 0, 0], [8192, 7, 7]], rt.STROKE_RADIUS_MAX, 3, shape=shape)) == 512
    # the figure of the contract
    assert len(check(ctx, [[0, 0, 0], [63, 63, 63]], 2, 6)) == 1186


def test_closed_loop_with_dabs(ctx):
    pts = np.array([[4, 4, 4], [26, 6, 9], [24, 27, 12], [5, 25, 20], [16, 16, 30], [40, 16, 16]], np.int32)
    seg = np.array([[0, 1], [1, 2], [4, 4], [2, 3], [3, 0], [5, 5], [1, 1]], np.uint32)
    mats = np.array([1, 2, 3, 4, 5, 6, 7], np.int32)
    for shape in NIBS:
        want = check(ctx, pts, 2, 5, segments=seg, materials=mats, shape=shape)
        assert set(want[:, 3]) == {1, 2, 3, 4, 5, 7}                       # point 5 lies off the grid: its dab adds nothing
        # the dab on point 1 comes last, so it owns its whole ball; an explicit empty list draws nothing
        ball = sm.voxelize(pts[1:2], 2, 5, shape=shape)
        assert (want[np.isin(sm.morton(want[:, :3]), sm.morton(ball[:, :3])), 3] == 7).all()
        assert ctx.voxelize_stroke(pts, 2, 5, segments=np.zeros((0, 2), np.uint32), shape=shape).shape == (0, 4)


# ---- 4. scan and search boundaries ---------------------------------------------------------------------------------------------
def short_segments(rng, count, n, big_ends=False):
    """count short segments scattered over the grid (some off it: no candidates); big_ends: the first and the last span it."""
    a = rng.integers(-4, n + 4, (count, 1, 3))
    pts = (a + rng.integers(-3, 4, (count, 2, 3))).astype(np.int32)
    if big_ends:
        pts[0] = [[0, 0, 0], [n - 1, n // 2, n - 1]]
        pts[-1] = [[n - 1, 0, 2], [0, n - 1, n // 3]]
    return pts.reshape(-1, 3), np.arange(2 * count, dtype=np.uint32).reshape(-1, 2)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_scan_and_search_boundaries(ctx, count):
    rng = np.random.default_rng(count)
    pts, seg = short_segments(rng, count, 64)
    if count == 1:
        pts[:] = [[20, 21, 22], [23, 20, 24]]
    mats = rng.integers(1, 255, count).astype(np.int32)
    shape = NIBS[count & 1]
    assert len(check(ctx, pts, 1, 6, segments=seg, materials=mats, shape=shape, tag=count)) > 0


def test_large_segments_first_and_last(ctx):
    rng = np.random.default_rng(5)
    pts, seg = short_segments(rng, 257, 64, big_ends=True)
    mats = rng.integers(1, 255, len(seg)).astype(np.int32)
    mats[0], mats[-1] = 100, 200
    for shape in NIBS:
        want = check(ctx, pts, 1, 6, segments=seg, materials=mats, shape=shape)
        assert (want[:, 3] == 200).sum() > 64 and (want[:, 3] == 100).sum() > 64


# ---- 5. the edit and extract forms ---------------------------------------------------------------------------------------------
def edit_stroke(depth, rng):
    """A stroke through a grid of side 2^depth: a polyline that enters and leaves it, a loop, and dabs; per-segment materials."""
    n = 1 << depth
    pts, mats = sm.random_stroke(rng, 12, n, reach=n // 4)
    seg = np.concatenate([sm.segments_of(len(pts)), [[12, 0], [5, 5], [2, 9]]]).astype(np.uint32)
    return pts, seg, rng.integers(1, 21, len(seg)).astype(np.int32)


def edit_cases(ctx, cells, depth, V, pts, seg, mats, shape, tag):
    """Every op: the edit form against expected bytes and against the two-call composition; extract against the model; undo."""
    r = 2
    B = sm.voxelize(pts, r, depth, seg, mats, shape=shape)
    assert len(B) > 0 and 0 < np.isin(sm.morton(B[:, :3]), sm.morton(V[:, :3])).sum() < len(B)
    for op in OPS:
        want_vox = apply_op(V, op, B, 0)
        built = built_cells(ctx, want_vox, depth)
        n_want = len(built) // 16
        room = max(len(cells) // 16, n_want) + 8
        vbo, counter = bind_cells(ctx, cells, room)
        n = ctx.octree_edit_stroke(op, pts, r, seg, mats, shape=shape)
        got = vbo.read(np.uint32)
        assert n == n_want and int(counter.read(np.uint32)[0]) == n, (tag, op)
        assert np.array_equal(got, padded(built, 64 * room)), (tag, op)
        vbo, counter = bind_cells(ctx, cells, room)
        assert ctx.octree_edit_voxels(op, ctx.voxelize_stroke(pts, r, depth, seg, mats, shape=shape)) == n
        assert np.array_equal(vbo.read(np.uint32), got), (tag, op)
    # the undo record: V's voxels under the stroke with V's materials; CLEAR, then SET of the record, restores the tree
    room = len(cells) // 16 + depth * len(B) + 64
    vbo, counter = bind_cells(ctx, cells, room)
    saved = ctx.octree_extract_stroke(pts, r, seg, shape=shape)
    assert np.array_equal(saved, sm.intersect(V, B)) and 0 < len(saved) < len(V), tag
    assert np.array_equal(vbo.read(np.uint32), padded(cells, 64 * room)) and int(counter.read(np.uint32)[0]) == 12345      # extract writes nothing
    canonical, n0 = expected_bytes(ctx, V, depth, 64 * room)
    ctx.octree_edit_stroke(rt.REGION_CLEAR, pts, r, seg, shape=shape)
    assert not np.array_equal(vbo.read(np.uint32), canonical)
    assert ctx.octree_edit_voxels(rt.REGION_SET, saved) == n0
    assert np.array_equal(vbo.read(np.uint32), canonical), tag


@pytest.mark.parametrize("shape", NIBS)
def test_edit_stroke_on_a_random_tree(ctx, shape):
    depth = 5
    rng = np.random.default_rng(40 + shape)
    centres = rng.integers(2, 30, (40, 3))
    vox = np.concatenate([block(c - rng.integers(0, 3, 3), c + rng.integers(0, 3, 3), int(rng.integers(1, 21))) for c in centres])
    vox = vox[((vox[:, :3] >= 0) & (vox[:, :3] < 32)).all(1)]
    _, first = np.unique(sm.morton(vox[:, :3]), return_index=True)
    vbo, counter, V = bind_tree(ctx, vox[np.sort(first)], depth)
    cells = vbo.read(np.uint32)
    pts, seg, mats = edit_stroke(depth, rng)
    edit_cases(ctx, cells, depth, V, pts, seg, mats, shape, "random")


@pytest.mark.parametrize("shape", NIBS)
def test_edit_stroke_on_a_hand_built_tree_with_merged_leaves(ctx, shape):
    depth = 4
    vox = np.concatenate([block((0, 0, 0), (15, 3, 15), 3), block((4, 4, 4), (11, 11, 11), 5), [[15, 15, 15, 7]]]).astype(np.int32)
    vbo, counter, V = bind_tree(ctx, vox, depth)
    cells = vbo.read(np.uint32)
    assert len(cells) // 16 < len(V) // 8                                  # merged LEAFs: far fewer cells than voxels
    pts, seg, mats = edit_stroke(depth, np.random.default_rng(44 + shape))
    edit_cases(ctx, cells, depth, V, pts, seg, mats, shape, "hand")


def test_a_dab_leaves_the_bytes_of_the_matching_region_edit(ctx):
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    ints = rt.VertexBufferObject(ctx, scene.blobs[7])
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
    room = len(cells) // 16 + 4096
    for c, r in (((30, 31, 29), 5), ((2, 60, 33), 4), ((70, 30, 30), 9)):
        for shape in NIBS:
            region = rt.sphere(c, r) if shape == rt.SHAPE_SPHERE else rt.box(tuple(v - r for v in c), tuple(v + r for v in c))
            for op in OPS:
                vbo, counter = bind_cells(ctx, cells, room)
                n1 = ctx.octree_edit_region(op, [region], 6)
                want = vbo.read(np.uint32)
                vbo, counter = bind_cells(ctx, cells, room)
                assert ctx.octree_edit_stroke(op, [c], r, material=6, shape=shape) == n1
                assert np.array_equal(vbo.read(np.uint32), want), (c, r, shape, op)


# ---- 6. errors leave every byte as it was ------------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    nc, nv = ctypes.c_uint32(0), ctypes.c_size_t(0)
    pts = np.array([[3, 4, 5], [20, 9, 12], [9, 30, 6]], np.int32)
    seg = np.array([[0, 1], [1, 2]], np.uint32)
    one = np.array([5, 6], np.int32)
    ok, keep = rt._stroke(pts, 2, seg, one)

    def raw(**f):
        """A tdt_stroke like `ok` but for the given fields (the Python wrapper would refuse most of these itself)."""
        s = rt.Stroke(ok.points, ok.segments, ok.materials, ok.n_points, ok.n_segments, ok.shape, ok.radius, ok.material, 0)
        for k, v in f.items():
            setattr(s, k, v)
        return s

    ctx = rt.Context(0)
    try:
        # unbound slots: the edit and extract forms
        for bound in ((), (0,), (7,)):
            for s in bound:
                b = rt.VertexBufferObject(ctx, cells if s == 0 else np.array([depth, 64, 128], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, b)
            assert L.tdt_octree_edit_stroke(ctx.h, 0, ctypes.byref(ok), ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract_stroke(ctx.h, ctypes.byref(ok), None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        assert len(ctx.voxelize_stroke(pts, 2, 5)) > 0             # needs no tree
        vbos = rt.upload_scene(ctx, scene)
        counter = rt.VertexBufferObject(ctx, np.array([777], np.uint32))
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)

        def unchanged():
            return np.array_equal(vbos[0].read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 777

        far, neg = pts.copy(), pts.copy()
        far[1, 2] = rt.STROKE_COORD_MAX + 1
        neg[2, 0] = -rt.STROKE_COORD_MAX - 1
        bad_seg = np.array([[0, 1], [1, 3]], np.uint32)
        m0, m255 = np.array([0, 5], np.int32), np.array([5, 255], np.int32)
        bad = [raw(points=far.ctypes.data), raw(points=neg.ctypes.data), raw(segments=bad_seg.ctypes.data),
               raw(materials=m0.ctypes.data), raw(materials=m255.ctypes.data), raw(materials=None, material=254), raw(materials=None, material=-1),
               raw(radius=-1), raw(radius=rt.STROKE_RADIUS_MAX + 1), raw(shape=2), raw(shape=-1), raw(pad=1),
               raw(points=None),                                   # NULL arrays with counts above 0
               raw(segments=None),                                 # segments == NULL with n_segments != 0
               raw(n_points=0, points=None),                       # n_points = 0 with segments
               raw(n_points=(1 << 20) + 1), raw(n_segments=(1 << 20) + 1)]
        out = np.zeros((4096, 4), np.int32)
        for i, s in enumerate(bad):
            for rc in (L.tdt_octree_edit_stroke(ctx.h, 0, ctypes.byref(s), ctypes.byref(nc)),
                       L.tdt_voxelize_stroke(ctx.h, ctypes.byref(s), 5, out.ctypes.data, len(out), ctypes.byref(nv)),
                       L.tdt_octree_extract_stroke(ctx.h, ctypes.byref(s), out.ctypes.data, len(out), ctypes.byref(nv))):
                assert rc == rt.ERR_INVALID_VALUE and unchanged() and not out.any() and nv.value == 0, i
        for rc in (L.tdt_octree_edit_stroke(ctx.h, 0, None, ctypes.byref(nc)), L.tdt_octree_edit_stroke(ctx.h, 4, ctypes.byref(ok), ctypes.byref(nc)),
                   L.tdt_octree_edit_stroke(ctx.h, -1, ctypes.byref(ok), ctypes.byref(nc)),
                   L.tdt_voxelize_stroke(ctx.h, None, 5, None, 0, ctypes.byref(nv)), L.tdt_voxelize_stroke(ctx.h, ctypes.byref(ok), 0, None, 0, ctypes.byref(nv)),
                   L.tdt_voxelize_stroke(ctx.h, ctypes.byref(ok), 11, None, 0, ctypes.byref(nv)), L.tdt_voxelize_stroke(ctx.h, ctypes.byref(ok), 5, None, 0, None),
                   L.tdt_octree_extract_stroke(ctx.h, None, None, 0, ctypes.byref(nv)), L.tdt_octree_extract_stroke(ctx.h, ctypes.byref(ok), None, 0, None)):
            assert rc == rt.ERR_INVALID_VALUE and unchanged()
        # what the wrapper refuses never reaches the library
        for f in (lambda: ctx.octree_edit_stroke(0, far, 2), lambda: ctx.voxelize_stroke(pts, 2, 11), lambda: ctx.octree_edit_stroke(4, pts, 2)):
            with pytest.raises(ValueError):
                f()
        assert unchanged()
        # extract forms: NULL counts only; a capacity below the count: the count, nothing written
        want = sm.voxelize(pts, 2, depth, seg, one)
        for fn, args, full in ((L.tdt_voxelize_stroke, (ctypes.byref(ok), depth), want),
                               (L.tdt_octree_extract_stroke, (ctypes.byref(ok),), sm.intersect(ctx.octree_extract(), want))):
            assert len(full) > 1
            assert fn(ctx.h, *args, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == len(full)
            out = np.zeros((len(full), 4), np.int32)
            nv = ctypes.c_size_t(0)
            assert fn(ctx.h, *args, out.ctypes.data, len(full) - 1, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
            assert nv.value == len(full) and not out.any()
            assert fn(ctx.h, *args, out.ctypes.data, len(full), ctypes.byref(nv)) == rt.OK and np.array_equal(out, full)
        assert unchanged()
        # limit 1, found on the host before anything is allocated: 40 grid-spanning segments of the largest radius at depth 10
        # are 40 * 128^3 tiles
        span = np.array([[0, 0, 0], [1023, 1023, 1023]], np.int32)
        seg40 = np.tile(np.array([[0, 1]], np.uint32), (40, 1))
        assert 40 * sm.tile_candidates(span[0], span[1], rt.STROKE_RADIUS_MAX, 10) == 40 << 21 > rt.REGION_BRUSH_CAP
        for shape in NIBS:
            with pytest.raises(rt.TdtError, match=str(40 << 21)) as e:
                ctx.voxelize_stroke(span, rt.STROKE_RADIUS_MAX, 10, seg40, shape=shape)
            assert e.value.code == rt.ERR_INVALID_VALUE
        vb10, counter10, _ = bind_tree(ctx, np.array([[1, 1, 1, 1], [1000, 2, 3, 4]], np.int32), 10)
        before = vb10.read(np.uint32)
        with pytest.raises(rt.TdtError, match=str(40 << 21)) as e:
            ctx.octree_edit_stroke(rt.REGION_SET, span, rt.STROKE_RADIUS_MAX, seg40)
        assert e.value.code == rt.ERR_INVALID_VALUE and np.array_equal(vb10.read(np.uint32), before)
        assert int(counter10.read(np.uint32)[0]) == 12345
        # limit 2, found by the counting pass: one dab of the largest radius in the middle of the depth-9 grid covers all 2^27
        # voxels; the same dab at depth 8 counts 2^24
        for shape in NIBS:
            with pytest.raises(rt.TdtError, match=str(1 << 27)) as e:
                ctx.voxelize_stroke([[256, 256, 256]], rt.STROKE_RADIUS_MAX, 9, shape=shape)
            assert e.value.code == rt.ERR_INVALID_VALUE
        dab, keep2 = rt._stroke([[128, 128, 128]], rt.STROKE_RADIUS_MAX)
        assert L.tdt_voxelize_stroke(ctx.h, ctypes.byref(dab), 8, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == 1 << 24
        # the empty stroke, and a stroke wholly off the grid: an empty list
        assert ctx.voxelize_stroke(np.zeros((0, 3), np.int32), 3, 4).shape == (0, 4)
        assert ctx.voxelize_stroke(pts - 100, 3, 4).shape == (0, 4)
        # a misfit: a buffer one cell too small reports the count it needs and keeps its bytes
        want = sm.voxelize(pts, 2, 5, seg, one)
        vbo, counter2, V1 = bind_tree(ctx, np.array([[3, 3, 3, 5]], np.int32), 5)
        chain = vbo.read(np.uint32)
        built = built_cells(ctx, apply_op(V1, rt.REGION_SET, want, 0), 5)
        need = len(built) // 16
        assert need > len(chain) // 16
        vbo, counter2 = bind_cells(ctx, chain, need - 1)
        with pytest.raises(rt.TdtError) as e:
            ctx.octree_edit_stroke(rt.REGION_SET, pts, 2, seg, one)
        assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
        assert np.array_equal(vbo.read(np.uint32), padded(chain, 64 * (need - 1))) and int(counter2.read(np.uint32)[0]) == 12345
        vbo, counter2 = bind_cells(ctx, chain, need)
        assert ctx.octree_edit_stroke(rt.REGION_SET, pts, 2, seg, one) == need and np.array_equal(vbo.read(np.uint32), built)
        # the empty stroke, edit form: an empty brush, i.e. the tree's compacted bytes
        vbo, counter2 = bind_cells(ctx, chain, need)
        assert ctx.octree_edit_stroke(rt.REGION_SET, np.zeros((0, 3), np.int32), 2) == len(chain) // 16
        assert np.array_equal(vbo.read(np.uint32), padded(chain, 64 * need))
        assert ctx.octree_extract_stroke(np.zeros((0, 3), np.int32), 2).shape == (0, 4)
        del keep, keep2
    finally:
        ctx.close()


# ---- 7. multi-device ---------------------------------------------------------------------------------------------------------
def test_multi_device_context():
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    scene.blobs[0] = padded(cells, 64 * (8 ** depth // 7 + 2))
    cam = host.camera_reference_pose(96, 64, 2, 3)
    pts, seg, mats = edit_stroke(depth, np.random.default_rng(9))
    outs = []
    for devices in (None, [0, 0]):                             # two members on one device: every replica path, on any machine
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            lst = r.ctx.voxelize_stroke(pts, 3, depth, seg, mats)
            saved = r.ctx.octree_extract_stroke(pts, 3, seg)
            before = r.vbos[0].read(np.uint32)
            zeros = np.zeros(len(seg), np.int32)
            zero = rt.Stroke(pts.ctypes.data, seg.ctypes.data, zeros.ctypes.data, len(pts), len(seg), rt.SHAPE_SPHERE, 3, 0, 0)
            nc = ctypes.c_uint32(0)
            assert rt.lib().tdt_octree_edit_stroke(r.ctx.h, rt.REGION_SET, ctypes.byref(zero), ctypes.byref(nc)) == rt.ERR_INVALID_VALUE
            assert np.array_equal(r.vbos[0].read(np.uint32), before)
            n = r.ctx.octree_edit_stroke(rt.REGION_SET, pts, 3, seg, mats)
            outs.append((n, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), lst, saved))
        finally:
            r.close()
    (n1, c1, img1, v1, l1, s1), (n2, c2, img2, v2, l2, s2) = outs
    assert n1 == n2 and np.array_equal(c1, c2) and np.array_equal(v1, v2) and np.array_equal(l1, l2) and np.array_equal(s1, s2)
    B = sm.voxelize(pts, 3, depth, seg, mats)
    assert np.array_equal(l1, B) and len(s1) > 0
    assert (img1.view(np.uint32) == img2.view(np.uint32)).all()


# ---- 8. the pixel forms ------------------------------------------------------------------------------------------------------
def pixel_path(w, h):
    """A drag across the frame that starts and ends off the model: the sky breaks it."""
    k = 24
    t = np.linspace(0.0, 1.0, k)
    return np.stack([np.rint(2 + t * (w - 5)), np.rint(h * 0.5 + (h * 0.45) * np.sin(t * 7.0))], 1).astype(np.int32)


def picked_stroke(r, px, op):
    """What Renderer.stroke must draw, from pick and the model: (one voxel or None per pixel, points, segments)."""
    place = 1 if op in (rt.REGION_SET, rt.REGION_FILL) else 0
    uniforms = (r.vbos[6].read(np.float32), r.vbos[7].read(np.int32))
    vox = []
    for h in r.pick(px):
        try:
            vox.append(host.pick_grid_voxel(h, uniforms, place))
        except ValueError:
            vox.append(None)
    return (vox,) + sm.stroke_from_picks(vox)


def check_picked(vox, seg):
    """The path has a miss inside it, joined runs and enough hits to draw something."""
    hit = np.array([v is not None for v in vox])
    assert hit.sum() >= 4 and (hit[1:] & hit[:-1]).any() and len(seg) >= 2
    first, last = np.flatnonzero(hit)[[0, -1]]
    assert (~hit[first:last]).any()


def test_renderer_stroke_on_the_demo_scene():
    """Scene.demo() is 19 shared cells that stand for 235 M voxels, and its canonical tree, which every region edit installs, takes
    35 M cells (2.2 GB): no test can afford that buffer, let alone the oracle's frame of it.  So on this scene the stroke is taken up
    to the install: the points and segments are the model's, the list is the model's, and the edit reports the misfit with the
    cell count to grow to and leaves every byte as it was.  The edit itself and its frame: the next test, on config 2."""
    w, h, radius = 96, 64, 3
    base = host.Scene.demo()
    depth = base.max_depth
    cells = np.ascontiguousarray(base.blobs[0]).view(np.uint32)
    cam = host.camera_reference_pose(w, h, 2, 3)
    px = pixel_path(w, h)
    r = rt.Renderer(base, cam)
    try:
        frame = r.render()
        vox, pts, seg = picked_stroke(r, px, rt.REGION_SET)
        check_picked(vox, seg)
        B = sm.voxelize(pts, radius, depth, seg, material=4)
        assert len(B) > 0 and np.array_equal(r.ctx.voxelize_stroke(pts, radius, depth, seg, material=4), B)
        with pytest.raises(rt.TdtError) as e:
            r.stroke(px, radius, rt.REGION_SET, material=4)
        assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells > 30_000_000
        assert np.array_equal(r.vbos[0].read(np.uint32), cells)
        assert (r.render().view(np.uint32) == frame.view(np.uint32)).all()
    finally:
        r.close()


@pytest.mark.parametrize("op,shape", [(rt.REGION_SET, rt.SHAPE_SPHERE), (rt.REGION_CLEAR, rt.SHAPE_BOX)])
def test_renderer_stroke_then_render(oracle, op, shape):
    w, h, radius = 96, 64, 3
    base = host.Scene.config(2)                                    # what the demo program draws in the suites' demo tests
    depth = base.max_depth
    room = 8 ** depth // 7 + 2                                      # no depth-6 tree has more cells
    scene = host.Scene({**base.blobs, 0: padded(np.ascontiguousarray(base.blobs[0]).view(np.uint32), 64 * room)})
    cam = host.camera_reference_pose(w, h, 2, 3)
    px = pixel_path(w, h)
    r = rt.Renderer(scene, cam)
    try:
        r.render()                                                  # derived tables of the tree as it was
        vox, pts, seg = picked_stroke(r, px, op)
        check_picked(vox, seg)
        V = r.ctx.octree_extract()
        B = sm.voxelize(pts, radius, depth, seg, material=4, shape=shape)
        ctx2 = rt.Context(0)
        try:
            want, n = expected_bytes(ctx2, apply_op(V, op, B, 0), depth, 64 * room)
        finally:
            ctx2.close()
        got_pts, cells = r.stroke(px, radius, op, material=4, shape=shape)
        assert got_pts.dtype == np.int32 and np.array_equal(got_pts, pts) and cells == n
        got = r.vbos[0].read(np.uint32)
        assert np.array_equal(got, want) and not np.array_equal(got, np.ascontiguousarray(scene.blobs[0]).view(np.uint32))
        img = r.render()
    finally:
        r.close()
    ref = oracle.render(host.Scene({**scene.blobs, 0: got}), cam, threads=4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


def test_demo_stroke_equals_the_python_call(tmp_path):
    exe = build.build_demo()
    w, h = 96, 64
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    room = 8 ** depth // 7 + 2
    cam = host.camera_reference_pose(w, h, 2, 3)                   # the demo's camera
    px = pixel_path(w, h)
    for nib, shape, op, name in (("sphere", rt.SHAPE_SPHERE, rt.REGION_SET, "set"), ("box", rt.SHAPE_BOX, rt.REGION_CLEAR, "clear")):
        out = str(tmp_path / f"{nib}.pfm")
        p = subprocess.run([exe, "--config", "2", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "3", "--cells", str(room), "--stroke",
                            ";".join(f"{x},{y}" for x, y in px), "--brush", f"{nib}:2", "--op", name, "--material", "6", "--out", out],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"stroke pixels (\d+) points (\d+):((?: -?\d+,-?\d+,-?\d+)*) op (\w+) cells (\d+)", p.stdout)
        assert m and int(m.group(1)) == len(px) and m.group(4) == name, p.stdout
        demo_pts = np.array([[int(c) for c in t.split(",")] for t in m.group(3).split()], np.int32).reshape(-1, 3)
        assert len(demo_pts) == int(m.group(2)) > 0
        r = rt.Renderer(host.Scene({**scene.blobs, 0: padded(cells, 64 * room)}), cam)
        try:
            pts, n = r.stroke(px, 2, op, material=6, shape=shape)
            img = r.render()
        finally:
            r.close()
        assert np.array_equal(pts, demo_pts) and n == int(m.group(5)), nib
        with open(out, "rb") as f:
            assert f.readline().strip() == b"PF4"
            fw, fh = map(int, f.readline().split())
            f.readline()
            frame = np.frombuffer(f.read(), "<f4").reshape(fh, fw, 4)
        assert (frame.view(np.uint32) == img.view(np.uint32)).all(), nib
