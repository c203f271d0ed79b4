"""Enclosed space on the GPU (tdt_octree_extract_enclosed / tdt_octree_fill_enclosed / tdt_voxelize_triangles_solid /
tdt_octree_edit_triangles_solid): the voxel lists must equal the numpy model (tests/fill_model.py: propagation from the grid's
faces on a dense grid) or the closed forms of the definition element for element, and the edit forms must leave in the bound
cells buffer exactly what tdt_octree_edit_voxels of those lists leaves."""
import ctypes
import functools
import re
import subprocess

import numpy as np
import pytest

import fill_model as fm
import mesh_model as mm
import oracle_py
from octree_util import distinct_deltas, edit_setup, expand_cells
from test_fill_api import hollow, without
from test_gpu_connect import bind_tree, block, serpentine
from test_gpu_mesh import CUBE_PLY
from test_gpu_region_edit import apply_op, bind_cells, built_cells, expected_bytes, padded, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
OPS = (rt.REGION_SET, rt.REGION_FILL, rt.REGION_PAINT, rt.REGION_CLEAR)
U = mm.UNIT


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def same(got, want, tag=""):
    assert got.shape == want.shape and np.array_equal(got, want), tag


def inner_of(lo, hi, m):
    """The inside of hollow(lo, hi): what a fill with inherited material adds."""
    return block(tuple(c + 1 for c in lo), tuple(c - 1 for c in hi), m)


# ---- 1. random trees ---------------------------------------------------------------------------------------------------------
# occupancy at which the model finds pockets: isolated empties need all 6 (26) neighbours solid
DENSITY = {6: 0.6, 26: 0.9}


def random_tree(depth, connectivity):
    rng = np.random.default_rng(1000 * depth + connectivity)
    n = 1 << depth
    p = np.argwhere(rng.random((n, n, n)) < DENSITY[connectivity])
    return sort_vox(np.concatenate([p, rng.integers(1, 255, (len(p), 1))], 1))


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("depth", [3, 4, 5, 6])
def test_random_trees_equal_the_model(ctx, depth, connectivity):
    n = 1 << depth
    V = random_tree(depth, connectivity)
    E = fm.enclosed_grid(V, depth, connectivity)
    want = fm.enclosed(V, depth, connectivity, E=E)
    assert 0 < len(want) < n ** 3 - len(V)                    # pockets exist, and some empty space drains: on the CPU, by the model alone
    assert len(set(want[:, 3])) > 1
    mask = [rt.box((1, 0, 2), (n // 2, n - 2, n - 1)), rt.sphere((n // 2, n // 2, n // 3), n // 3)]
    masked = fm.enclosed(V, depth, connectivity, regions=mask, E=E)
    assert 0 < len(masked) and (len(masked) < len(want) or depth == 3)
    bind_tree(ctx, V, depth)
    same(ctx.octree_extract_enclosed(connectivity), want, "inherit")
    same(ctx.octree_extract_enclosed(connectivity, 17), fm.enclosed(V, depth, connectivity, 17, E=E), "fixed")
    same(ctx.octree_extract_enclosed(connectivity, None, mask), masked, "inherit, masked")
    same(ctx.octree_extract_enclosed(connectivity, 253, mask), fm.enclosed(V, depth, connectivity, 253, mask, E=E), "fixed, masked")
    assert len(ctx.octree_extract_enclosed(connectivity, None, [])) == 0          # an empty mask
    same(ctx.octree_extract(), V, "the tree is untouched")


# ---- 2. word and tile boundaries ---------------------------------------------------------------------------------------------
EDGES = (0, 1, 31, 32, 33, 62, 63, 64, 65, 126, 127)


def boundary_boxes(depth, axis, inner_only):
    """Hollow boxes, inner width 1 and 2 along `axis`, one wall at each coordinate of EDGES along it (the low wall where the box
    then fits, the high wall otherwise), spread over the two other axes so that no two touch; material = 1 + its number."""
    n = 1 << depth
    out = []
    coords = [c for c in EDGES if c < n and not (inner_only and c in (0, n - 1))]
    for c in coords:
        for width in (1, 2):
            k = len(out)
            lo_a = c if c + width + 1 <= n - 1 else c - width - 1
            lo, hi = [0, 0, 0], [0, 0, 0]
            lo[axis], hi[axis] = lo_a, lo_a + width + 1
            for j, other in enumerate(a for a in range(3) if a != axis):
                slot = (k % 5, k // 5)[j]
                lo[other] = 3 + 7 * slot + (k % 3)
                hi[other] = lo[other] + 2 + (k + j) % 2         # inner 1 or 2 across
            out.append((tuple(lo), tuple(hi), 1 + k))
    return out


@pytest.mark.parametrize("inner_only", [True, False])
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("depth", [6, 7])
def test_word_and_tile_boundaries(ctx, depth, axis, inner_only):
    n = 1 << depth
    boxes = boundary_boxes(depth, axis, inner_only)
    V = sort_vox(np.concatenate([hollow(lo, hi, m) for lo, hi, m in boxes]))
    lo, hi = V[:, :3].min(0), V[:, :3].max(0)
    if inner_only:                                             # bbox(V) is neither word-aligned nor a multiple of the tile:
        for a in (1, 2):                                       # a lone voxel past the boxes stretches it where it would be
            if (hi[a] - lo[a] + 1) % 8 == 0:
                pebble = lo.copy()
                pebble[a] = hi[a] + 2
                V = sort_vox(np.concatenate([V, [[*pebble, 200]]]))
        lo, hi = V[:, :3].min(0), V[:, :3].max(0)
        assert lo[0] % 32 and (hi[0] + 1) % 32 and (hi[1] - lo[1] + 1) % 8 and (hi[2] - lo[2] + 1) % 8
    assert len(np.unique(V[:, :3], axis=0)) == len(V) and V[:, :3].max() < n
    want = sort_vox(np.concatenate([inner_of(lo, hi, m) for lo, hi, m in boxes]))
    if depth == 6:
        same(fm.enclosed(V, depth), want, "the closed form is the model's")
    bind_tree(ctx, V, depth)
    for conn in (6, 26):
        same(ctx.octree_extract_enclosed(conn), want, conn)
    # with one box's wall opened in the middle of a face, exactly that box drains
    lo0, hi0, _ = boxes[len(boxes) // 2]
    hole = [lo0[a] + 1 for a in range(3)]
    hole[(axis + 1) % 3] = lo0[(axis + 1) % 3]
    bind_tree(ctx, without(V, hole), depth)
    rest = sort_vox(np.concatenate([inner_of(lo, hi, m) for i, (lo, hi, m) in enumerate(boxes) if i != len(boxes) // 2]))
    same(ctx.octree_extract_enclosed(6), rest, "one box open")


# ---- 3. convergence ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[6, 7])
def corridor(request):
    """A one-voxel-wide corridor winding through every 8 x 8 tile of rows, inside solid rock filling the grid: (depth, the
    corridor's voxels in walking order, the rock)."""
    depth = request.param
    n = 1 << depth
    path = serpentine(n - 2)[:, :3] + 1                        # coordinates 1 .. n - 2: no corridor voxel on a grid face
    rock = np.ones((n, n, n), bool)
    rock[path[:, 0], path[:, 1], path[:, 2]] = False
    assert rock[0].all() and rock[-1].all() and rock[:, 0].all() and rock[:, -1].all() and rock[:, :, 0].all() and rock[:, :, -1].all()
    tiles = {(y // 8, z // 8) for _, y, z in path}
    assert len(tiles) == (n // 8) ** 2                         # every tile of rows
    return depth, path, rock


def rock_list(rock, material=4):
    p = np.argwhere(rock)
    return sort_vox(np.concatenate([p, np.full((len(p), 1), material)], 1))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_corridor_sealed_and_open(ctx, corridor, connectivity):
    depth, path, rock = corridor
    # sealed: the whole corridor is enclosed, and nothing else
    bind_tree(ctx, rock_list(rock), depth)
    got = ctx.octree_extract_enclosed(connectivity, 8)
    assert len(got) == len(path)
    same(got, sort_vox(np.concatenate([path, np.full((len(path), 1), 9)], 1)), "sealed")
    # open at one end only: the flood has to walk the whole corridor, and nothing may remain
    x, y, z = path[0]
    assert x == 1
    rock = rock.copy()
    rock[0, y, z] = False                                      # a door in the face x = 0
    bind_tree(ctx, rock_list(rock), depth)
    assert len(ctx.octree_extract_enclosed(connectivity)) == 0
    assert ctx.fill_passes() > (1 << depth) // 8               # it took more than one sweep of tiles
    # open at the far end instead
    rock[0, y, z] = True
    x, y, z = path[-1]
    door = [(x, y, zz) for zz in range(z + 1, 1 << depth)]      # straight out through the rock above it
    assert all(rock[d] for d in door)
    for d in door:
        rock[d] = False
    bind_tree(ctx, rock_list(rock), depth)
    assert len(ctx.octree_extract_enclosed(connectivity)) == 0


# ---- 4. leaks ----------------------------------------------------------------------------------------------------------------
def test_leaks_and_nested_shells(ctx):
    depth = 5
    lo, hi = (5, 6, 7), (20, 17, 15)
    W = hollow(lo, hi, 3)
    inside = (hi[0] - lo[0] - 1) * (hi[1] - lo[1] - 1) * (hi[2] - lo[2] - 1)
    cases = {
        "closed": (W, inside, inside),
        "face hole": (without(W, (12, 6, 11)), 0, 0),
        "edge gap": (without(W, (5, 6, 10)), inside, 0),
        "corner gap": (without(W, (20, 17, 15)), inside, 0),
    }
    for name, (vox, want6, want26) in cases.items():
        bind_tree(ctx, vox, depth)
        for conn, want in ((6, want6), (26, want26)):
            got = ctx.octree_extract_enclosed(conn)
            assert len(got) == want, (name, conn)
            same(got, fm.enclosed(vox, depth, conn), (name, conn))
    # a cavity that reaches a grid face: the box's wall on the face y = 31 is missing
    open_box = hollow((3, 20, 3), (12, 31, 12), 2)
    open_box = open_box[open_box[:, 1] < 31]
    bind_tree(ctx, open_box, depth)
    assert len(ctx.octree_extract_enclosed(6)) == 0 and len(fm.enclosed(open_box, depth)) == 0
    # the same box closed BY a wall lying on the face: enclosed
    closed = hollow((3, 20, 3), (12, 31, 12), 2)
    bind_tree(ctx, closed, depth)
    assert len(ctx.octree_extract_enclosed(26)) == 8 * 10 * 8
    # nested shells: the gap between them and the inner cavity both fill, each from its own wall
    outer, inner = hollow((2, 2, 2), (29, 29, 29), 10), hollow((9, 9, 9), (22, 22, 22), 20)
    nested = np.concatenate([outer, inner, [[15, 15, 15, 30]]])
    want = fm.enclosed(nested, depth)
    assert len(want) == 26 ** 3 - 14 ** 3 + 12 ** 3 - 1 and set(want[:, 3]) == {10, 20, 30}
    bind_tree(ctx, nested, depth)
    for conn in (6, 26):
        same(ctx.octree_extract_enclosed(conn), want, conn)


# ---- 5. extremes -------------------------------------------------------------------------------------------------------------
def test_extremes(ctx):
    for name, vox, depth in (("empty", np.zeros((0, 4), np.int32), 4), ("full", block((0, 0, 0), (15, 15, 15), 2), 4),
                             ("one voxel", np.array([[7, 8, 9, 5]], np.int32), 4), ("depth 1", block((0, 0, 0), (1, 1, 0), 3), 1),
                             ("depth 1 full", block((0, 0, 0), (1, 1, 1), 3), 1), ("a plate", block((3, 0, 2), (3, 15, 14), 3), 4),
                             ("two plates", np.concatenate([block((3, 0, 2), (3, 15, 14), 3), block((5, 0, 2), (5, 15, 14), 3)]), 4)):
        bind_tree(ctx, vox, depth, room=4)
        before = ctx._keep[0].read(np.uint32)
        for conn in (6, 26):
            assert len(ctx.octree_extract_enclosed(conn)) == 0, name
        # the edit form of an empty E installs the compacted bytes: these trees are canonical already
        assert ctx.octree_fill_enclosed() == max(len(before) // 16 - 4, 1) and np.array_equal(ctx._keep[0].read(np.uint32), before), name
    # a full tree with one voxel missing inside, and one missing on a face
    full = block((0, 0, 0), (15, 15, 15), 2)
    bind_tree(ctx, without(full, (8, 7, 6), (15, 3, 3)), 4)
    assert ctx.octree_extract_enclosed(26).tolist() == [[8, 7, 6, 2]]          # the rock's material + 1, inherited


def test_depth10_small_box_far_from_the_origin(ctx):
    lo, hi = (1000, 1000, 1000), (1004, 1004, 1004)
    W = hollow(lo, hi, 0)
    W[:, 3] = 1 + (W[:, 1] - 1000) * 5 + (W[:, 2] - 1000)      # the -x wall's material names the row
    bind_tree(ctx, W, 10)
    want = inner_of(lo, hi, 0)
    want[:, 3] = 1 + (want[:, 1] - 1000) * 5 + (want[:, 2] - 1000)
    for conn in (6, 26):
        same(ctx.octree_extract_enclosed(conn), sort_vox(want), conn)
    # two such boxes at opposite corners: the bit volume spans the whole grid (2^30 bits)
    far = hollow((2, 3, 4), (6, 7, 8), 200)
    bind_tree(ctx, np.concatenate([W, far]), 10)
    same(ctx.octree_extract_enclosed(6), sort_vox(np.concatenate([want, inner_of((2, 3, 4), (6, 7, 8), 200)])), "whole grid")


def test_merged_leaf_tree_config2():
    scene = host.Scene.config(2)
    depth = scene.max_depth
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        assert np.array_equal(V, sort_vox(expand_cells(scene.blobs[0], depth)))
        for conn in (6, 26):
            same(ctx.octree_extract_enclosed(conn), fm.enclosed(V, depth, conn), ("config2", conn))
        # hollowed, every merged block has an inside again
        S = ctx.octree_extract_morph(rt.MORPH_SHELL, 1)
        del vbos
        bind_tree(ctx, S, depth)
        want = fm.enclosed(S, depth)
        assert 0 < len(want) and np.isin(fm.keys(want[:, :3]), fm.keys(V[:, :3])).sum() > 0
        same(ctx.octree_extract_enclosed(6), want, "config2 hollowed")
    finally:
        ctx.close()


# ---- 6. the edit form --------------------------------------------------------------------------------------------------------
def hollowed_config2(ctx):
    """config 2 with its solids hollowed (MORPH_SHELL, radius 1, the 26-neighbourhood: the shells are tight under 26 too):
    (scene, depth, the voxel list)."""
    scene = host.Scene.config(2)
    vbos = rt.upload_scene(ctx, scene)
    S = ctx.octree_extract_morph(rt.MORPH_SHELL, 1, 26)
    del vbos
    return scene, scene.max_depth, S


def test_fill_bytes_undo_and_render(oracle):
    cam = host.camera_reference_pose(96, 64, 2, 3)
    ctx = rt.Context(0)
    try:
        scene, depth, S = hollowed_config2(ctx)
        mask = [rt.sphere((32, 32, 32), 20)]
        results = {}
        for name, conn, material, regions in (("inherit", 6, None, None), ("fixed 26", 26, 11, None), ("masked", 6, 5, mask)):
            E = fm.enclosed(S, depth, conn, material, regions)
            assert len(E) > 0
            want_vox = apply_op(S, rt.REGION_FILL, E, 0)
            same(want_vox, fm.filled(S, depth, conn, material, regions), name)
            built = built_cells(ctx, want_vox, depth)
            original = built_cells(ctx, S, depth)
            room = max(len(built), len(original)) // 16 + 8
            vbo, counter = bind_cells(ctx, original, room)
            v7 = rt.VertexBufferObject(ctx, scene.blobs[7])
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, v7)
            saved = ctx.octree_extract_enclosed(conn, material, regions)
            same(saved, E, name)
            n = ctx.octree_fill_enclosed(conn, material, regions)
            assert n == len(built) // 16 and int(counter.read(np.uint32)[0]) == n, name
            assert np.array_equal(vbo.read(np.uint32), padded(built, 64 * room)), name
            results[name] = vbo.read(np.uint32)
            if regions is None:
                assert len(ctx.octree_extract_enclosed(conn)) == 0            # nothing is left to fill
            # undo
            n = ctx.octree_edit_voxels(rt.REGION_CLEAR, saved)
            assert n == len(original) // 16 and int(counter.read(np.uint32)[0]) == n
            assert np.array_equal(vbo.read(np.uint32), padded(original, 64 * room)), name
    finally:
        ctx.close()
    # one small frame after a fill, against the oracle on the same cells
    room = len(results["inherit"]) // 16
    r = rt.Renderer(host.Scene({**scene.blobs, 0: padded(built_cells_of(S, depth), 64 * room)}), cam)
    try:
        r.render()                                              # derived tables of the tree as it was
        r.ctx.octree_fill_enclosed()
        got = r.vbos[0].read(np.uint32)
        img = r.render()
    finally:
        r.close()
    assert np.array_equal(got, results["inherit"])
    ref = oracle.render(host.Scene({**scene.blobs, 0: got}), cam, threads=4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


def built_cells_of(vox, depth):
    ctx = rt.Context(0)
    try:
        return built_cells(ctx, vox, depth)
    finally:
        ctx.close()


def test_edit_dispatched_just_before_is_included(oracle):
    ctx = rt.Context(0)
    try:
        scene, depth, S = hollowed_config2(ctx)
        cells = built_cells(ctx, S, depth)
    finally:
        ctx.close()
    used = len(cells) // 16
    scene.blobs[0] = np.concatenate([cells, np.zeros(16 * 34000, np.uint32)])
    d = distinct_deltas(np.random.default_rng(21), 200, depth, scene.blobs[0])
    d[:, 3], d[:, 4] = 2.0, 4.0
    edited, _ = oracle_py.oracle_octree_update(oracle, scene, d, used, (len(d), 1, 1))
    r, upd, counter = edit_setup(scene, used, d)
    try:
        ctx2 = rt.Context(0)
        try:
            bind_cells(ctx2, edited, len(edited) // 16)
            v7 = rt.VertexBufferObject(ctx2, scene.blobs[7])
            ctx2.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, v7)
            V = ctx2.octree_extract()
            E = fm.enclosed(V, depth)
            assert len(V) > len(S) and 0 < len(E) != len(fm.enclosed(S, depth))       # the edit placed voxels, some of them in cavities
            want, n_want = expected_bytes(ctx2, apply_op(V, rt.REGION_FILL, E, 0), depth, scene.blobs[0].nbytes)
        finally:
            ctx2.close()
        upd.dispatch_compute(len(d), 1, 1)                     # no finish
        n = r.ctx.octree_fill_enclosed()
        assert n == n_want and np.array_equal(r.vbos[0].read(np.uint32), want)
        assert int(counter.read(np.uint32)[0]) == n
    finally:
        r.close()


def test_errors_write_nothing():
    L = rt.lib()
    ctx = rt.Context(0)
    nc, nv = ctypes.c_uint32(0), ctypes.c_size_t(0)
    ok = rt.Fill(6, -1)
    v = (np.array([[1, 1, 1], [9, 2, 1], [4, 8, 6], [5, 4, 9]]) * U).astype(np.int32)
    t = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3]], np.uint32)
    mesh, keep = rt._mesh(v, t, None, 0)
    try:
        # unbound slots: the tree forms and the mesh edit form
        cells0 = built_cells(ctx, hollow((1, 1, 1), (5, 5, 5)), 4)
        for bound in ((), (0,), (7,)):
            for s in bound:
                b = rt.VertexBufferObject(ctx, cells0 if s == 0 else np.array([4, 64, 16], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, b)
            assert L.tdt_octree_fill_enclosed(ctx.h, ctypes.byref(ok), None, 0, ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract_enclosed(ctx.h, ctypes.byref(ok), None, 0, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_edit_triangles_solid(ctx.h, 0, ctypes.byref(mesh), ctypes.byref(ok), ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        assert len(ctx.voxelize_triangles_solid(v, t, 4)) > 0     # needs no tree
        W = np.concatenate([hollow((1, 1, 1), (6, 6, 6), 3), hollow((8, 8, 8), (14, 13, 12), 4)])
        vbo, counter, V = bind_tree(ctx, W, 4, room=2)
        before = vbo.read(np.uint32)

        def unchanged():
            return np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345

        X, F, MX, ME = ctx.octree_extract_enclosed, ctx.octree_fill_enclosed, ctx.voxelize_triangles_solid, ctx.octree_edit_triangles_solid
        bad_shape = rt.Region(2, (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(1, 1, 1), 0)
        far = v.copy()
        far[1, 2] = rt.MESH_COORD_MAX + 1
        cases = [lambda: X(7), lambda: F(7), lambda: X(0), lambda: F(18), lambda: X(6, 254), lambda: F(6, 254), lambda: X(6, -2), lambda: F(6, -2),
                 lambda: X(6, None, bad_shape), lambda: F(6, None, bad_shape), lambda: F(6, None, rt.sphere((3, 3, 3), -1)),
                 lambda: MX(v, t, 4, connectivity=8), lambda: ME(0, v, t, connectivity=8), lambda: MX(v, t, 4, fill_material=254),
                 lambda: ME(0, v, t, fill_material=-2), lambda: MX(v, t, 0), lambda: MX(v, t, 11), lambda: ME(4, v, t), lambda: ME(-1, v, t),
                 lambda: MX(v, np.array([[0, 1, 4]], np.uint32), 4), lambda: ME(0, v, np.array([[0, 1, 4]], np.uint32)),
                 lambda: MX(far, t, 4), lambda: ME(0, far, t), lambda: ME(0, v, t, [0, 1, 1, 1]), lambda: MX(v, t, 4, None, 254)]
        for i, f in enumerate(cases):
            with pytest.raises(rt.TdtError) as e:
                f()
            assert e.value.code == rt.ERR_INVALID_VALUE and unchanged(), i
        one = rt.Region(rt.SHAPE_BOX, (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(9, 9, 9), 0)
        for rc in (L.tdt_octree_fill_enclosed(ctx.h, None, None, 0, ctypes.byref(nc)),
                   L.tdt_octree_extract_enclosed(ctx.h, None, None, 0, None, 0, ctypes.byref(nv)),
                   L.tdt_octree_fill_enclosed(ctx.h, ctypes.byref(ok), None, 1, ctypes.byref(nc)),
                   L.tdt_octree_extract_enclosed(ctx.h, ctypes.byref(ok), None, 1, None, 0, ctypes.byref(nv)),
                   L.tdt_octree_extract_enclosed(ctx.h, ctypes.byref(ok), ctypes.byref(one), 1, None, 0, None),
                   L.tdt_voxelize_triangles_solid(ctx.h, ctypes.byref(mesh), 4, None, None, 0, ctypes.byref(nv)),
                   L.tdt_voxelize_triangles_solid(ctx.h, None, 4, ctypes.byref(ok), None, 0, ctypes.byref(nv)),
                   L.tdt_voxelize_triangles_solid(ctx.h, ctypes.byref(mesh), 4, ctypes.byref(ok), None, 0, None),
                   L.tdt_octree_edit_triangles_solid(ctx.h, 0, ctypes.byref(mesh), None, ctypes.byref(nc)),
                   L.tdt_octree_edit_triangles_solid(ctx.h, 0, None, ctypes.byref(ok), ctypes.byref(nc))):
            assert rc == rt.ERR_INVALID_VALUE and unchanged()
        # extract form: NULL counts only; a capacity below the count: the count, nothing written
        want = fm.enclosed(V, 4)
        assert L.tdt_octree_extract_enclosed(ctx.h, ctypes.byref(ok), None, 0, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == len(want) > 0
        out = np.zeros((len(want), 4), np.int32)
        nv = ctypes.c_size_t(0)
        assert L.tdt_octree_extract_enclosed(ctx.h, ctypes.byref(ok), None, 0, out.ctypes.data, len(want) - 1, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
        assert nv.value == len(want) and not out.any() and unchanged()
        assert L.tdt_octree_extract_enclosed(ctx.h, ctypes.byref(ok), None, 0, out.ctypes.data, len(want), ctypes.byref(nv)) == rt.OK
        assert np.array_equal(out, want) and unchanged()
        # a LEAF value >= 254
        leafy = before.copy()
        nodes = leafy.reshape(-1, 8, 2)
        i, j = np.argwhere(nodes[..., 1] == 2)[0]
        nodes[i, j, 0] = 254
        vbo2, counter2 = bind_cells(ctx, leafy, len(leafy) // 16)
        for f in (lambda: X(6), lambda: F(6)):
            with pytest.raises(rt.TdtError) as e:
                f()
            assert e.value.code == rt.ERR_INVALID_VALUE and np.array_equal(vbo2.read(np.uint32), leafy) and int(counter2.read(np.uint32)[0]) == 12345
        # a misfit: a buffer one cell too small reports the count it needs and keeps its bytes
        # (a whole fill never grows a canonical tree: an all-EMPTY block becomes one LEAF; a mask that cuts through blocks does)
        cut = rt.box((3, 3, 3), (4, 12, 12))
        cells = built_cells(ctx, V, 4)
        built = built_cells(ctx, fm.filled(V, 4, 6, 9, cut), 4)
        need = len(built) // 16
        assert need > len(cells) // 16
        vbo3, counter3 = bind_cells(ctx, cells, need - 1)
        with pytest.raises(rt.TdtError) as e:
            F(6, 9, cut)
        assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
        assert np.array_equal(vbo3.read(np.uint32), padded(cells, 64 * (need - 1))) and int(counter3.read(np.uint32)[0]) == 12345
        vbo3, counter3 = bind_cells(ctx, cells, need)
        assert F(6, 9, cut) == need and np.array_equal(vbo3.read(np.uint32), built) and int(counter3.read(np.uint32)[0]) == need
        del keep
    finally:
        ctx.close()


def shell_voxels(lo, hi, m):
    """hollow(lo, hi, m) for boxes too large to enumerate whole: the six faces, each built as a plane."""
    faces = []
    for a in range(3):
        u, w = [b for b in range(3) if b != a]
        g = np.stack(np.meshgrid(np.arange(lo[u], hi[u] + 1), np.arange(lo[w], hi[w] + 1), indexing="ij"), -1).reshape(-1, 2)
        for c in (lo[a], hi[a]):
            f = np.empty((len(g), 3), np.int64)
            f[:, a], f[:, u], f[:, w] = c, g[:, 0], g[:, 1]
            faces.append(f)
    p = np.unique(np.concatenate(faces), axis=0)
    return np.concatenate([p, np.full((len(p), 1), m)], 1).astype(np.int32)


def test_voxel_caps_write_nothing():
    """|V|, |E| and |S| above 2^26 (TDT_REGION_BRUSH_CAP): TDT_ERR_INVALID_VALUE, buffer and counter as they were."""
    cap = rt.REGION_BRUSH_CAP
    lo, hi = (50, 50, 50), (458, 458, 458)                     # inner side 407: 407^3 = 67 419 143 > 2^26 = 67 108 864
    assert (hi[0] - lo[0] - 1) ** 3 > cap
    ctx = rt.Context(0)
    try:
        X, F, MX, ME = ctx.octree_extract_enclosed, ctx.octree_fill_enclosed, ctx.voxelize_triangles_solid, ctx.octree_edit_triangles_solid

        def refused(calls, vbo, counter, before, text):
            for i, f in enumerate(calls):
                with pytest.raises(rt.TdtError, match=text) as e:
                    f()
                assert e.value.code == rt.ERR_INVALID_VALUE, i
                assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345, i

        # |V|: a depth-9 tree whose root cell is eight merged LEAFs holds 2^27 voxels in one cell
        root = np.zeros((8, 2), np.uint32)
        root[:, 0], root[:, 1] = 3, 2
        vbo, counter = bind_cells(ctx, root.reshape(-1), 1)
        ints = rt.VertexBufferObject(ctx, np.array([9, 64, 512], np.int32))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
        assert ctx._voxel_count() == 2 * cap
        refused([lambda: X(6), lambda: F(6), lambda: X(26, 4), lambda: F(26, 4)], vbo, counter, root.reshape(-1), str(2 * cap))
        # |E|: a depth-9 hollow box, a million wall voxels around 407^3 empty ones
        W = shell_voxels(lo, hi, 5)
        vbo, counter, V = bind_tree(ctx, W, 9, room=2)
        before = vbo.read(np.uint32)
        refused([lambda: X(6), lambda: F(6), lambda: X(26, 7), lambda: F(26, 7)], vbo, counter, before, str(407 ** 3))
        # the cap is on what is reported: under a mask the same tree answers
        small = ctx.octree_extract_enclosed(6, None, rt.box((51, 51, 51), (60, 60, 52)))
        assert len(small) == 10 * 10 * 2 and set(small[:, 3]) == {5}
        # |E| of a mesh: the same box as twelve triangles
        v, t = cube_mesh(tuple(c * U + 20 for c in lo), tuple(c * U + 40 for c in hi))
        refused([lambda: MX(v, t, 9), lambda: ME(rt.REGION_SET, v, t), lambda: ME(rt.REGION_CLEAR, v, t, None, 0, 26, 9)], vbo, counter, before,
                str(407 ** 3))
        # |S| cannot exceed 2^26 on its own: the mesh unit refuses a mesh above 2^26 candidate tiles or covered (triangle, voxel)
        # pairs first, and the unique voxels are no more than the pairs; the solid forms hand that refusal on
        seg = np.array([[0, 0, 0], [1024 * U, 1024 * U, 1024 * U], [0, 0, 0]], np.int32)
        t33 = np.tile(np.array([[0, 1, 2]], np.uint32), (33, 1))
        with pytest.raises(rt.TdtError, match=str(33 << 21)) as e:
            MX(seg, t33, 10)
        assert e.value.code == rt.ERR_INVALID_VALUE and np.array_equal(vbo.read(np.uint32), before)
    finally:
        ctx.close()


def test_multi_device_context():
    cam = host.camera_reference_pose(96, 64, 2, 3)
    ctx = rt.Context(0)
    try:
        scene, depth, S = hollowed_config2(ctx)
        cells = built_cells(ctx, S, depth)
    finally:
        ctx.close()
    scene.blobs[0] = padded(cells, 64 * (8 ** depth // 7 + 2))
    sv, st = mm.uv_sphere((30.2, 33.1, 28.7), 14.3, 8, 10)
    v = host.mesh_quantize(sv)
    outs = []
    for devices in (None, [0, 0]):                             # two members on one device: every replica path, on any machine
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            lst = r.ctx.octree_extract_enclosed(6)
            solid = r.ctx.voxelize_triangles_solid(v, st, depth, None, 4)
            before = r.vbos[0].read(np.uint32)
            with pytest.raises(rt.TdtError):
                r.ctx.octree_fill_enclosed(9)
            with pytest.raises(rt.TdtError):
                r.ctx.octree_edit_triangles_solid(rt.REGION_SET, v, st, None, 4, 6, 254)
            assert np.array_equal(r.vbos[0].read(np.uint32), before)
            n1 = r.ctx.octree_fill_enclosed(6)
            mid = r.vbos[0].read(np.uint32)
            n2 = r.ctx.octree_edit_triangles_solid(rt.REGION_CLEAR, v, st, None, 4)
            outs.append((n1, n2, mid, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), lst, solid))
        finally:
            r.close()
    a, b = outs
    assert a[0] == b[0] and a[1] == b[1]
    for i in (2, 3, 5, 6, 7):
        assert np.array_equal(a[i], b[i]), i
    assert np.array_equal(a[6], fm.enclosed(S, depth)) and len(a[6]) > 0
    assert np.array_equal(a[5], apply_op(fm.filled(S, depth), rt.REGION_CLEAR, a[7], 0))
    assert (a[4].view(np.uint32) == b[4].view(np.uint32)).all()


# ---- 7. the mesh forms -------------------------------------------------------------------------------------------------------
def closed_meshes(depth):
    n = 1 << depth
    sv, st = mm.uv_sphere((n * 0.52, n * 0.47, n * 0.5), n * 0.37, 9, 12)
    tv, tt = mm.torus((n * 0.5, n * 0.5, n * 0.45), n * 0.3, n * 0.13, 14, 9)
    return {"uv_sphere": (host.mesh_quantize(sv), st), "torus": (host.mesh_quantize(tv), tt)}


@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("name", ["uv_sphere", "torus"])
def test_solid_meshes_equal_the_model(ctx, name, depth):
    v, t = closed_meshes(depth)[name]
    mats = np.random.default_rng(depth).integers(1, 255, len(t)).astype(np.int32)
    S = mm.voxelize(v, t, depth, mats)
    for conn in (6, 26):
        want = fm.filled(S, depth, conn)
        assert len(want) > len(S) + (1 << depth)               # a real inside
        same(ctx.voxelize_triangles_solid(v, t, depth, mats, 0, conn), want, (name, conn))
    same(ctx.voxelize_triangles_solid(v, t, depth, None, 3, 6, 40), fm.filled(mm.voxelize(v, t, depth, None, 3), depth, 6, 40), "fixed")
    same(ctx.voxelize_triangles(v, t, depth, mats), S, "the surface form is unchanged")


def cube_mesh(lo, hi):
    v = np.array([(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.int64)
    t = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)],
                 np.uint32)
    return v.astype(np.int32), t


def test_mesh_materials_open_meshes_and_the_grid_faces(ctx):
    depth = 5
    # a cube with per-triangle materials: the inside inherits from the x = lo face, two triangles, two materials
    v, t = cube_mesh((5 * U + 7, 6 * U + 9, 4 * U + 30), (25 * U + 11, 22 * U + 40, 27 * U + 5))
    mats = np.arange(1, 13, dtype=np.int32) * 7
    S = mm.voxelize(v, t, depth, mats)
    want = fm.filled(S, depth)
    inner = want[~np.isin(fm.keys(want[:, :3]), fm.keys(S[:, :3]))]
    assert len(inner) == 19 * 15 * 22 and len(set(inner[:, 3])) >= 2
    same(ctx.voxelize_triangles_solid(v, t, depth, mats), want, "cube")
    # a sphere with its top stacks removed is a bowl: nothing is enclosed, the solid list is the surface list
    sv, st = mm.uv_sphere((16.3, 15.8, 15.1), 11.4, 9, 12)
    q = host.mesh_quantize(sv)
    top = sv[st].mean(1)[:, 2] > 15.1 + 11.4 * 0.55
    assert 0 < top.sum() < len(st)
    bowl = st[~top]
    surface = mm.voxelize(q, bowl, depth)
    assert len(fm.filled(mm.voxelize(q, st, depth), depth)) > len(mm.voxelize(q, st, depth))      # the whole sphere does enclose
    for conn in (6, 26):
        same(ctx.voxelize_triangles_solid(q, bowl, depth, connectivity=conn), surface, ("bowl", conn))
    # a sphere half outside the grid: what is left of its surface is open at the face x = 0
    hv, ht = mm.uv_sphere((0.4, 16.2, 15.7), 9.3, 9, 12)
    qh = host.mesh_quantize(hv)
    half = mm.voxelize(qh, ht, depth)
    assert len(half) > 0 and qh[:, 0].min() < 0
    same(ctx.voxelize_triangles_solid(qh, ht, depth), half, "half outside")
    same(half, fm.filled(half, depth), "the model agrees")
    # an empty mesh, and one wholly off the grid
    assert ctx.voxelize_triangles_solid(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), depth).shape == (0, 4)
    assert ctx.voxelize_triangles_solid(v + 40 * U, t, depth).shape == (0, 4)


def test_edit_triangles_solid_on_config2():
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    sv, st = mm.uv_sphere((30.2, 33.1, 28.7), 17.3, 9, 12)
    v = host.mesh_quantize(sv)
    mats = np.random.default_rng(7).integers(1, 21, len(st)).astype(np.int32)
    B = fm.filled(mm.voxelize(v, st, depth, mats), depth, 26)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        del vbos
        assert 0 < np.isin(fm.keys(B[:, :3]), fm.keys(V[:, :3])).sum() < len(B)
        v7 = rt.VertexBufferObject(ctx, scene.blobs[7])
        for op in OPS:
            built = built_cells(ctx, apply_op(V, op, B, 0), depth)
            n_want = len(built) // 16
            room = max(len(cells) // 16, n_want) + 8
            vbo, counter = bind_cells(ctx, cells, room)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, v7)
            n = ctx.octree_edit_triangles_solid(op, v, st, mats, 0, 26)
            assert n == n_want and int(counter.read(np.uint32)[0]) == n, op
            assert np.array_equal(vbo.read(np.uint32), padded(built, 64 * room)), op
    finally:
        ctx.close()


# ---- 8. the demo -------------------------------------------------------------------------------------------------------------
def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF4"
        w, h = map(int, f.readline().split())
        f.readline()
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 4)


def test_demo_solid_mesh_and_fill_enclosed(oracle, tmp_path):
    exe = build.build_demo()
    ply = tmp_path / "cube.ply"
    ply.write_text(CUBE_PLY)
    w, h = 96, 64
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    cam = host.camera_reference_pose(w, h, 2, 3)
    lo, hi = (20, 30, 10), (43, 49, 33)
    mesh = host.PlyMesh(ply.read_bytes())
    scale, off = host.mesh_fit(mesh.vertices, lo, hi)
    q = host.mesh_quantize(mesh.vertices, scale, off)
    B = fm.filled(mm.voxelize(q, mesh.triangles, depth, None, 6), depth)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        S = ctx.octree_extract_morph(rt.MORPH_SHELL, 1, 26)     # the demo's --conn is --morph's too
        del vbos
        stamped = built_cells(ctx, apply_op(V, rt.REGION_SET, B, 0), depth)
        E = fm.enclosed(S, depth, 26, 4)
        refilled = built_cells(ctx, apply_op(S, rt.REGION_FILL, E, 0), depth)
    finally:
        ctx.close()
    assert len(B) > len(mm.voxelize(q, mesh.triangles, depth)) and len(E) > 0
    room = max(len(cells), len(stamped), len(refilled)) // 16 + 8
    common = [exe, "--config", "2", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "3", "--cells", str(room)]
    out = str(tmp_path / "solid.pfm")
    p = subprocess.run(common + ["--mesh", str(ply), "--solid", "--material", "6", "--box", ",".join(str(c) for c in lo + hi), "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"mesh triangles 12 voxels {len(B)} solid op set cells {len(stamped) // 16}\b", p.stdout), p.stdout
    ref = oracle.render(host.Scene({**scene.blobs, 0: padded(stamped, 64 * room)}), cam, threads=8)
    assert (read_pfm(out).view(np.uint32) == ref.view(np.uint32)).all()
    out = str(tmp_path / "fill.pfm")
    p = subprocess.run(common + ["--morph", "shell:1", "--fill-enclosed", "--conn", "26", "--material", "4", "--out", out], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"fill-enclosed conn 26 voxels {len(E)} cells {len(refilled) // 16}\b", p.stdout), p.stdout
    ref = oracle.render(host.Scene({**scene.blobs, 0: padded(refilled, 64 * room)}), cam, threads=8)
    assert (read_pfm(out).view(np.uint32) == ref.view(np.uint32)).all()


# ---- 9. a list longer than one trip of the bounding box's strided loop ---------------------------------------------------------
BBOX_LAUNCH = 256 * 256                                        # lanes of tdt_bitvol.hip's bounding-box launch: a lane's first trip covers these


@functools.lru_cache(maxsize=None)
def strided_bbox_tree():
    """(depth, V, the voxels the shell encloses): a shell two voxels thick from (8,8,8) to (119,119,119), its cavity (10..117)^3,
    and two stray voxels in far corners of the grid, one material throughout.  Made once; callers do not write to it."""
    depth, m = 7, 6
    shell = block((8, 8, 8), (119, 119, 119), m)
    shell = shell[((shell[:, :3] < 10) | (shell[:, :3] > 117)).any(1)]
    V = sort_vox(np.concatenate([shell, [[127, 127, 0, m], [127, 127, 127, m]]]))
    V.setflags(write=False)
    return depth, V, block((10, 10, 10), (117, 117, 117), m)


def test_bounding_box_of_a_list_longer_than_its_launch(ctx):
    """bbox(V) needs the later trips of the strided loop: one axis minimum and one axis maximum lie beyond the first 65 536
    voxels of the Morton-sorted list, so a kernel that stopped after a lane's first voxel would size the volume wrongly."""
    depth, V, inside = strided_bbox_tree()
    assert len(V) == 145218 > 2 * BBOX_LAUNCH
    head = V[:BBOX_LAUNCH, :3]
    assert (head[:, 0].min(), head[:, 0].max(), head[:, 2].min(), head[:, 2].max()) == (8, 63, 8, 119)
    assert (V[:, 0].min(), V[:, 0].max(), V[:, 2].min(), V[:, 2].max()) == (8, 127, 0, 127)
    want = {conn: fm.enclosed(V, depth, conn) for conn in (6, 26)}
    for conn in (6, 26):
        assert len(want[conn]) == 108 ** 3
        same(want[conn], sort_vox(inside), "the cavity, whole")
    bind_tree(ctx, V, depth)
    for conn in (6, 26):
        same(ctx.octree_extract_enclosed(conn), want[conn], conn)
    same(ctx.octree_extract(), V, "the tree is untouched")
