"""Surface extraction on the GPU (tdt_octree_extract_surface): every result must equal the numpy model (tests/surface_model.py)
as bytes, content and order — on random trees, on runs and stacks that cross Morton blocks, at the grid's faces and at depth 10,
at the tile sizes of the device scan and sort, on merged LEAFs, under masks, after a queued edit, with the count / capacity rules
of tdt_octree_extract, with every error writing nothing, on a multi-device context, and end to end: the extracted surface
voxelised again gives the dilated solid, and the demo writes the same mesh as a PLY."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import fill_model as fm
import oracle_py
import surface_model as sm
from octree_util import distinct_deltas, edit_setup
from test_gpu_connect import bind_tree, block, hand_trees
from test_gpu_region_edit import bind_cells, built_cells, padded, sort_vox
from test_surface_api import MODES, random_grid
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
TILE = 2048                                                 # kScanTile = kSortTile


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def same(got, want, tag=""):
    assert got.dtype == want.dtype == np.int32 and got.shape == want.shape, (tag, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), tag


def check(ctx, vox, depth, regions=None, modes=MODES, tag=""):
    """Every mode on the builder's tree of vox against the model; the cells buffer and the counter must stay as they were."""
    vbo, counter, V = bind_tree(ctx, vox, depth)
    before = vbo.read(np.uint32)
    out = {}
    for merge, by_material in modes:
        got = ctx.octree_extract_surface(merge, by_material, regions)
        same(got, sm.quads(V, depth, merge, by_material, regions), (tag, merge, by_material))
        out[(merge, by_material)] = got
    assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345, tag
    return out


# ---- 1. random trees ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [2, 3, 5, 6])
def test_random_trees_equal_the_model(ctx, depth):
    rng = np.random.default_rng(600 + depth)
    V = random_grid(rng, depth, 0.45, materials=4 if depth < 6 else 254)
    out = check(ctx, V, depth, tag=depth)
    assert len(out[(1, 0)]) <= len(out[(1, 1)]) < len(out[(0, 1)]) == len(out[(0, 0)])       # merging merges, materials split


# ---- 2. runs and stacks across Morton blocks; the grid's faces -----------------------------------------------------------------
def test_rows_and_plates_cross_morton_blocks(ctx):
    row = block((0, 9, 17), (31, 9, 17), 3)
    out = check(ctx, row, 5, tag="row")
    assert len(out[(1, 1)]) == 6 and len(out[(0, 1)]) == 4 * 32 + 2
    plate = block((0, 0, 13), (31, 31, 13), 7)
    out = check(ctx, plate, 5, tag="plate")
    assert len(out[(1, 1)]) == 6 and sorted((out[(1, 1)][:, 5] * out[(1, 1)][:, 6]).tolist()) == [32] * 4 + [1024] * 2
    for axis in (0, 1):                                        # the same plate standing on its other axes
        p = plate.copy()
        p[:, [axis, 2]] = p[:, [2, axis]]
        assert len(check(ctx, p, 5, tag=("plate", axis))[(1, 1)]) == 6
    both = np.concatenate([row, plate, block((5, 5, 14), (20, 9, 14), 7), block((8, 12, 14), (11, 30, 15), 9)])
    check(ctx, both, 5, tag="row, plate and steps")


def test_grid_faces_and_the_full_grid(ctx):
    n = 16
    faces = np.array([[0, 5, 5, 1], [n - 1, 5, 5, 1], [5, 0, 5, 2], [5, n - 1, 5, 2], [5, 5, 0, 3], [5, 5, n - 1, 3], [0, 0, 0, 4],
                      [n - 1, n - 1, n - 1, 4], [0, n - 1, 0, 5], [n - 1, 0, n - 1, 5]], np.int32)
    check(ctx, faces, 4, tag="faces")
    shell = block((0, 0, 0), (n - 1, n - 1, n - 1), 6)
    shell = shell[((shell[:, :3] == 0) | (shell[:, :3] == n - 1)).any(1)]
    out = check(ctx, shell, 4, tag="shell")
    assert len(out[(1, 1)]) == 12                              # the grid's six faces and the cavity's six walls
    out = check(ctx, block((0, 0, 0), (31, 31, 31), 2), 5, tag="full")     # one root of merged LEAFs
    assert out[(1, 1)][:, 2:7].tolist() == [[0, 0, 0, 32, 32], [32, 0, 0, 32, 32], [0, 0, 0, 32, 32], [0, 32, 0, 32, 32], [0, 0, 0, 32, 32],
                                            [0, 0, 32, 32, 32]]


def test_depth_10_uses_every_key_bit(ctx):
    N = 1024
    vox = [[0, 0, 0, 1], [N - 1, N - 1, N - 1, 254]]
    vox += [[x, 700, 300, 9] for x in range(N - 5, N)]        # rows ending at 1023 along x, y and z: u of the z, x and y faces
    vox += [[300, y, 700, 8] for y in range(N - 4, N)]
    vox += [[700, 300, z, 7] for z in range(N - 3, N)]
    vox += [[N - 1, y, N - 2, 6] for y in range(N - 6, N - 1)]
    out = check(ctx, np.array(vox, np.int32), 10, tag="depth 10")
    q = out[(1, 1)]
    assert q[:, 2:5].max() == N and ((q[:, 0] == 1) & (q[:, 2] == N)).any()        # the plane at 1024
    assert (q[:, 5:7].max(1) == 5).sum() >= 4


# ---- 3. the tiles of the scan and the sort -------------------------------------------------------------------------------------
def lattice(count, stride=(2, 2)):
    """`count` positions of the plane z = 6 of a 256^2 grid, at the given strides along x and y."""
    i = np.arange(count)
    per_row = 256 // stride[0]
    return np.stack([(i % per_row) * stride[0], (i // per_row) * stride[1], np.full(count, 6)], 1)


@pytest.mark.parametrize("count", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_scan_and_sort_tiles(ctx, count):
    # isolated voxels: `count` faces, runs and quads in every direction
    p = lattice(count)
    V = sort_vox(np.concatenate([p, 1 + (np.arange(count)[:, None] % 5)], 1))
    assert (sm.exposed(V, 8).sum(0) == count).all()
    out = check(ctx, V, 8, modes=[(0, 1), (1, 1)], tag=("isolated", count))
    assert len(out[(1, 1)]) == len(out[(0, 1)]) == 6 * count
    # dominoes along x: 2 count faces in four directions; for +-z (u = x) count runs of two, for +-y (v = x) 2 count runs stacked
    # in pairs, so `count` runs and `count` quads in some directions, 2 count in others
    p = lattice(count, (3, 2))
    p = np.concatenate([p, p + (1, 0, 0)])
    V = sort_vox(np.concatenate([p, np.ones((len(p), 1), np.int64)], 1))
    assert sm.exposed(V, 8).sum(0).tolist() == [count, count, 2 * count, 2 * count, 2 * count, 2 * count]
    out = check(ctx, V, 8, modes=[(1, 1)], tag=("dominoes", count))
    assert len(out[(1, 1)]) == 6 * count and sorted(set(map(tuple, out[(1, 1)][:, 5:7].tolist()))) == [(1, 1), (1, 2), (2, 1)]


# ---- 4. merged LEAFs -------------------------------------------------------------------------------------------------------------
def test_merged_leaf_trees():
    ctx = rt.Context(0)
    try:
        vox, depth = hand_trees()["leaf_and_voxel"][:2]
        check(ctx, vox, depth, tag="leaf_and_voxel")
        scene = host.Scene.config(2)                               # the library's own tree: merged LEAFs, shared cells
        vbos = rt.upload_scene(ctx, scene)
        cells = vbos[0].read(np.uint32)
        V = ctx.octree_extract()
        assert len(V) > (np.asarray(scene.blobs[0]).view(np.uint32)[1::2] == 2).sum()        # some LEAF holds more than a voxel
        for merge, by_material in MODES:
            same(ctx.octree_extract_surface(merge, by_material), sm.quads(V, scene.max_depth, merge, by_material), (merge, by_material))
        assert np.array_equal(vbos[0].read(np.uint32), cells)
        del vbos
    finally:
        ctx.close()


# ---- 5. masks --------------------------------------------------------------------------------------------------------------------
def test_masks(ctx):
    plate = block((2, 3, 9), (28, 27, 9), 5)
    cut = rt.box((0, 0, 0), (11, 31, 31))
    out = check(ctx, plate, 5, regions=cut, tag="box")
    top = out[(1, 1)][out[(1, 1)][:, 0] == 5]
    assert top[:, 2:7].tolist() == [[2, 3, 10, 10, 25]]           # cut at the box: x 2..11, not at a run's end
    two = [rt.box((0, 0, 0), (11, 31, 31)), rt.box((20, 10, 0), (40, 12, 31))]
    out = check(ctx, plate, 5, regions=two, tag="two boxes")
    assert (out[(1, 1)][:, 0] == 5).sum() == 2
    rng = np.random.default_rng(8)
    V = random_grid(rng, 5, 0.5)
    check(ctx, V, 5, regions=rt.sphere((14, 17, 12), 9), tag="sphere")
    check(ctx, V, 5, regions=[rt.sphere((3, 3, 3), 6), rt.box((16, -5, 20), (99, 40, 25))], tag="sphere and box")
    assert ctx.octree_extract_surface(regions=[]).shape == (0, 8)
    assert ctx.octree_extract_surface(regions=rt.box((5, 5, 5), (4, 9, 9))).shape == (0, 8)


# ---- 6. ordering: directly after a queued edit -------------------------------------------------------------------------------------
def test_edit_dispatched_just_before_is_included(oracle):
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), np.zeros(16 * 4000, np.uint32)])
    d = distinct_deltas(np.random.default_rng(29), 200, depth, scene.blobs[0])
    d[:, 3], d[:, 4] = 2.0, 4.0
    edited, _ = oracle_py.oracle_octree_update(oracle, scene, d, used, (len(d), 1, 1))
    r, upd, counter = edit_setup(scene, used, d)
    try:
        before = r.ctx.octree_extract_surface()
        ctx2 = rt.Context(0)
        try:
            bind_cells(ctx2, edited, len(edited) // 16)
            v7 = rt.VertexBufferObject(ctx2, scene.blobs[7])
            ctx2.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, v7)
            want = sm.quads(ctx2.octree_extract(), depth)
        finally:
            ctx2.close()
        assert want.tobytes() != before.tobytes()
        upd.dispatch_compute(len(d), 1, 1)                     # no finish
        same(r.ctx.octree_extract_surface(), want)
    finally:
        r.close()


# ---- 7. count only, exact capacity, capacity - 1 -----------------------------------------------------------------------------------
def test_count_and_capacity_rules(ctx):
    L = rt.lib()
    rng = np.random.default_rng(12)
    vbo, counter, V = bind_tree(ctx, random_grid(rng, 4, 0.4), 4)
    before = vbo.read(np.uint32)
    for merge, by_material in MODES:
        want = sm.quads(V, 4, merge, by_material)
        opt = rt.Surface(merge, by_material)
        n = ctypes.c_size_t(0)
        assert L.tdt_octree_extract_surface(ctx.h, ctypes.byref(opt), None, 0, None, 0, ctypes.byref(n)) == rt.OK and n.value == len(want) > 0
        assert L.tdt_octree_extract_surface(ctx.h, ctypes.byref(opt), None, 0, None, 10 ** 6, ctypes.byref(n)) == rt.OK and n.value == len(want)
        out = np.full((len(want) + 1, 8), 0x5A5A5A5A, np.int32)
        n = ctypes.c_size_t(0)
        assert L.tdt_octree_extract_surface(ctx.h, ctypes.byref(opt), None, 0, out.ctypes.data, len(want) - 1, ctypes.byref(n)) == rt.ERR_INVALID_VALUE
        assert n.value == len(want) and (out == 0x5A5A5A5A).all()
        n = ctypes.c_size_t(0)
        assert L.tdt_octree_extract_surface(ctx.h, ctypes.byref(opt), None, 0, out.ctypes.data, len(want), ctypes.byref(n)) == rt.OK
        assert n.value == len(want) and out[:-1].tobytes() == want.tobytes() and (out[-1] == 0x5A5A5A5A).all()
        assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345
    # an empty tree
    bind_tree(ctx, np.zeros((0, 4), np.int32), 3)
    assert ctx.octree_extract_surface().shape == (0, 8)


# ---- 8. errors leave every byte as it was ------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    ctx = rt.Context(0)
    ok = rt.Surface(1, 1)
    n = ctypes.c_size_t(0)
    out = np.full((64, 8), 0x5A5A5A5A, np.int32)
    try:
        cells0 = built_cells(ctx, block((1, 1, 1), (5, 5, 5)), 4)
        for bound in ((), (0,), (7,)):
            for s in bound:
                b = rt.VertexBufferObject(ctx, cells0 if s == 0 else np.array([4, 64, 16], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, b)
            assert L.tdt_octree_extract_surface(ctx.h, ctypes.byref(ok), None, 0, out.ctypes.data, 64, ctypes.byref(n)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        vbo, counter, V = bind_tree(ctx, np.concatenate([block((1, 1, 1), (5, 5, 5), 3), block((8, 8, 8), (9, 13, 12), 4)]), 4)
        before = vbo.read(np.uint32)
        assert len(sm.quads(V, 4)) <= 64

        def unchanged():
            return np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345 and (out == 0x5A5A5A5A).all()

        X = ctx.octree_extract_surface
        bad_shape = rt.Region(2, (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(1, 1, 1), 0)
        for i, f in enumerate([lambda: X(2), lambda: X(-1), lambda: X(1, 2), lambda: X(0, -1), lambda: X(regions=bad_shape),
                               lambda: X(regions=rt.sphere((3, 3, 3), -1)), lambda: X(regions=[rt.box((0, 0, 0), (3, 3, 3)), bad_shape])]):
            with pytest.raises(rt.TdtError) as e:
                f()
            assert e.value.code == rt.ERR_INVALID_VALUE and unchanged(), i
        one = rt.box((0, 0, 0), (9, 9, 9))
        for opt in (rt.Surface(2, 1), rt.Surface(1, -1), rt.Surface(-1, 0), rt.Surface(0, 2)):
            assert L.tdt_octree_extract_surface(ctx.h, ctypes.byref(opt), None, 0, out.ctypes.data, 64, ctypes.byref(n)) == rt.ERR_INVALID_VALUE
            assert unchanged()
        for rc in (L.tdt_octree_extract_surface(ctx.h, None, None, 0, out.ctypes.data, 64, ctypes.byref(n)),
                   L.tdt_octree_extract_surface(ctx.h, ctypes.byref(ok), None, 1, out.ctypes.data, 64, ctypes.byref(n)),
                   L.tdt_octree_extract_surface(ctx.h, ctypes.byref(ok), ctypes.byref(one), 1, out.ctypes.data, 64, None)):
            assert rc == rt.ERR_INVALID_VALUE and unchanged()
        # a LEAF value >= 254
        leafy = before.copy()
        nodes = leafy.reshape(-1, 8, 2)
        i, j = np.argwhere(nodes[..., 1] == 2)[0]
        nodes[i, j, 0] = 254
        vbo2, counter2 = bind_cells(ctx, leafy, len(leafy) // 16)
        with pytest.raises(rt.TdtError) as e:
            X()
        assert e.value.code == rt.ERR_INVALID_VALUE and np.array_equal(vbo2.read(np.uint32), leafy) and int(counter2.read(np.uint32)[0]) == 12345
        assert L.tdt_octree_extract_surface(ctx.h, ctypes.byref(ok), None, 0, out.ctypes.data, 64, ctypes.byref(n)) == rt.ERR_INVALID_VALUE
        assert (out == 0x5A5A5A5A).all()
        # |V| above 2^26: a depth-9 tree whose root cell is eight merged LEAFs holds 2^27 voxels in one cell
        root = np.zeros((8, 2), np.uint32)
        root[:, 0], root[:, 1] = 3, 2
        vbo3, counter3 = bind_cells(ctx, root.reshape(-1), 1)
        ints = rt.VertexBufferObject(ctx, np.array([9, 64, 512], np.int32))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
        for merge in (0, 1):
            with pytest.raises(rt.TdtError, match=str(2 * rt.REGION_BRUSH_CAP)) as e:
                X(merge)
            assert e.value.code == rt.ERR_INVALID_VALUE
            assert np.array_equal(vbo3.read(np.uint32), root.reshape(-1)) and int(counter3.read(np.uint32)[0]) == 12345
        # Python-side checks raise before the call
        with pytest.raises(ValueError):
            X(merge=2 ** 32 + 1)
    finally:
        ctx.close()


# ---- 9. multi-device ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0], [0, 1]])
def test_multi_device_context_answers_from_the_first_device(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("fewer than two devices are visible")
    scene = host.Scene.config(2)
    cam = host.camera_reference_pose(64, 48, 1, 2)
    outs = []
    for dev in (None, devices):
        r = rt.Renderer(scene, cam, devices=dev)
        try:
            c = r.ctx.octree_extract()[7, :3].astype(int)
            outs.append([r.ctx.octree_extract_surface(m, b, reg) for m, b in MODES for reg in (None, [rt.sphere(c, 14)])])
            cells = r.vbos[0].read(np.uint32)
            assert np.array_equal(cells[: len(np.asarray(scene.blobs[0]).view(np.uint32).ravel())], np.asarray(scene.blobs[0]).view(np.uint32).ravel())
        finally:
            r.close()
    for a, b in zip(*outs):
        assert len(a) and a.tobytes() == b.tobytes()


# ---- 10. end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", [0, 1])
def test_surface_voxelised_again_is_the_dilated_solid(ctx, merge):
    depth = 6
    vbo, counter = bind_cells(ctx, np.zeros(16, np.uint32), 40000)
    ints = rt.VertexBufferObject(ctx, np.array([depth, 64, 1 << depth], np.int32))
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
    ctx.octree_edit_region(rt.REGION_SET, [rt.sphere((24, 30, 28), 13)], 3)
    ctx.octree_edit_region(rt.REGION_SET, [rt.box((30, 20, 22), (52, 41, 37))], 8)
    ctx.octree_edit_region(rt.REGION_CLEAR, [rt.box((34, 24, 26), (45, 36, 33))], 0)          # a cavity: its walls are surface too
    V = ctx.octree_extract()
    assert len(V) > 5000 and V[:, :3].min() >= 1 and V[:, :3].max() <= (1 << depth) - 2       # strictly inside the grid
    Q = ctx.octree_extract_surface(merge, False)
    same(Q, sm.quads(V, depth, merge, False))
    vert, tri, _ = host.quads_to_mesh(Q)
    got = ctx.voxelize_triangles_solid(vert, tri, depth)
    want = fm.filled(ctx.octree_extract_morph(rt.MORPH_DILATE, 1, 26), depth, fast=True)
    assert np.array_equal(fm.keys(got[:, :3]), fm.keys(want[:, :3]))
    del ints


def test_demo_exports_the_same_mesh(tmp_path):
    exe = build.build_demo()
    out = str(tmp_path / "surface.ply")
    scene = host.Scene.config(2)
    n = 1 << scene.max_depth
    lo, hi = (n // 4, n // 4, n // 4), (n // 2, n // 2 + 3, n // 2 + 1)
    ctx = rt.Context(0)
    try:
        blobs = dict(scene.blobs)
        blobs[0] = padded(np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), 64 * 40000)
        vbos = rt.upload_scene(ctx, host.Scene(blobs))
        ctx.octree_edit_region(rt.REGION_SET, [rt.box(lo, hi)], 5)
        want = {}
        for merge, by_material in ((1, 1), (0, 0)):
            Q = ctx.octree_extract_surface(merge, by_material, [rt.box((0, 0, 0), (n - 1, n - 1, n // 2))])
            same(Q, sm.quads(ctx.octree_extract(), scene.max_depth, merge, by_material, [rt.box((0, 0, 0), (n - 1, n - 1, n // 2))]))
            want[(merge, by_material)] = (len(Q),) + host.quads_to_mesh(Q)[:2]
        del vbos
    finally:
        ctx.close()
    for (merge, by_material), (nq, vert, tri) in want.items():
        flags = ([] if merge else ["--no-merge"]) + ([] if by_material else ["--any-material"])
        p = subprocess.run([exe, "--config", "2", "--size", "32x24", "--spp", "1", "--bounce", "1", "--cells", "40000", "--box",
                            ",".join(map(str, lo + hi)), "--op", "set", "--material", "5", "--export-mesh", out, "--mask",
                            f"0,0,0,{n - 1},{n - 1},{n // 2}"] + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert re.search(rf"export-mesh (merged|unmerged)( any-material)? quads {nq} vertices {len(vert)} triangles {len(tri)}\b", p.stdout), p.stdout
        back = host.PlyMesh(open(out, "rb").read())
        assert np.array_equal(host.mesh_quantize(back.vertices), vert) and np.array_equal(back.triangles, tri)
