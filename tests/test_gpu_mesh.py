"""Triangle-mesh voxelisation (tdt_voxelize_triangles / tdt_octree_edit_triangles): the voxel list must equal the numpy model
(tests/mesh_model.py: the 13-axis test in int64, highest triangle wins) bit for bit, and the edit form must leave in the bound
cells buffer exactly what tdt_octree_edit_voxels of that list leaves — the builder's tree of op(V, list) followed by zeros."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import mesh_model as mm
import oracle_py
from octree_util import distinct_deltas, edit_setup
from test_gpu_connect import bind_tree, block
from test_gpu_region_edit import apply_op, bind_cells, built_cells, expected_bytes, padded
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
OPS = (rt.REGION_SET, rt.REGION_FILL, rt.REGION_PAINT, rt.REGION_CLEAR)
U = mm.UNIT


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def check(ctx, v, t, depth, materials=None, material=0, tag="", model=mm.voxelize):
    want = model(v, t, depth, materials, material)
    got = ctx.voxelize_triangles(v, t, depth, materials, material)
    assert got.shape == want.shape and np.array_equal(got, want), tag
    return want


# ---- 1. random meshes of the six kinds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 5, 6])
def test_extract_equals_the_model(ctx, depth):
    rng = np.random.default_rng(100 + depth)
    n = 1 << depth
    v, t, kinds = mm.random_triangles(rng, 204, n)
    mats = rng.integers(1, 255, len(t)).astype(np.int32)
    want = check(ctx, v, t, depth, mats)
    assert len(want) > 0 and set(kinds) == set(mm.KINDS)
    # clipping happens on all six grid faces
    assert (v.min(0) < 0).all() and (v.max(0) > n * U).all()
    for a in range(3):
        assert want[:, a].min() == 0 and want[:, a].max() == n - 1
    # the tie rule is exercised: some voxel is covered by two or more triangles of different materials
    per = [mm.voxelize(v, t[i:i + 1], depth, mats[i:i + 1]) for i in range(len(t))]
    allv = np.concatenate(per)
    key = mm.morton(allv[:, :3])
    order = np.argsort(key, kind="stable")
    key, m = key[order], allv[order, 3]
    same = key[1:] == key[:-1]
    assert (same & (m[1:] != m[:-1])).any()
    # the uniform-material form
    check(ctx, v, t, depth, None, 17)


# ---- 2. tile boundaries ------------------------------------------------------------------------------------------------------
def test_tile_boundaries(ctx):
    tri = np.array([[0, 1, 2]], np.uint32)
    # in the plane x = 8 voxels: the voxels of both tiles next to it
    v = np.array([[8 * U, 2 * U + 5, 3 * U + 7], [8 * U, 6 * U + 1, 3 * U + 9], [8 * U, 3 * U, 7 * U - 3]], np.int32)
    got = check(ctx, v, tri, 5)
    assert set(got[:, 0]) == {7, 8} and (got[got[:, 0] == 7][:, 1:3] == got[got[:, 0] == 8][:, 1:3]).all()
    # a vertex exactly on a tile corner: it touches eight tiles
    v = np.array([[8 * U, 8 * U, 8 * U], [9 * U + 3, 10 * U + 1, 9 * U + 11], [10 * U + 2, 9 * U + 5, 11 * U]], np.int32)
    got = check(ctx, v, tri, 4)
    assert {(x, y, z) for x in (7, 8) for y in (7, 8) for z in (7, 8)} <= {tuple(p) for p in got[:, :3]}
    # inside a single voxel
    v = np.array([[5 * U + 3, 9 * U + 4, 2 * U + 5], [5 * U + 60, 9 * U + 9, 2 * U + 50], [5 * U + 9, 9 * U + 61, 2 * U + 30]], np.int32)
    got = check(ctx, v, tri, 4, material=3)
    assert got.tolist() == [[5, 9, 2, 4]]
    # exactly one tile: two triangles in the plane z = 8.5 voxels over the open interior of tile (1, 0, 1) at depth 5
    q = np.array([[8 * U + 1, 1, 8 * U + 32], [16 * U - 1, 1, 8 * U + 32], [16 * U - 1, 8 * U - 1, 8 * U + 32], [8 * U + 1, 8 * U - 1, 8 * U + 32]], np.int32)
    got = check(ctx, q, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), 5)
    assert len(got) == 64 and set(got[:, 0] // 8) == {1} and set(got[:, 1] // 8) == {0} and set(got[:, 2]) == {8}
    # a slab that IS one whole tile: a diagonal through it and its faces' planes
    v = np.array([[8 * U, 8 * U, 8 * U], [16 * U, 16 * U, 16 * U], [16 * U, 8 * U, 16 * U]], np.int32)
    assert len(check(ctx, v, tri, 5)) > 0


# ---- 3. scan and search boundaries -------------------------------------------------------------------------------------------
def small_mesh(rng, count, n, big_ends=False):
    """count small triangles scattered over the grid (some off it: no candidates); big_ends: the first and the last span it."""
    a = rng.integers(-U, (n + 1) * U, (count, 1, 3))
    v = (a + rng.integers(-U, U + 1, (count, 3, 3))).astype(np.int32)
    if big_ends:
        v[0] = [[0, 0, 0], [n * U, n * U // 2, n * U], [n * U // 2, n * U, n * U]]
        v[-1] = [[n * U, 0, 0], [0, n * U, n * U // 3], [0, n * U // 2, n * U]]
    return v.reshape(-1, 3), np.arange(3 * count, dtype=np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 1025, 2047, 2048, 2049])
def test_scan_and_search_boundaries(ctx, count):
    rng = np.random.default_rng(count)
    v, t = small_mesh(rng, count, 64)
    mats = rng.integers(1, 255, count).astype(np.int32)
    # (the batched form of the model: tests/test_mesh_api.py pins it to the per-triangle one)
    assert len(check(ctx, v, t, 6, mats, tag=count, model=mm.voxelize_many)) > 0


def test_large_triangles_first_and_last(ctx):
    rng = np.random.default_rng(5)
    v, t = small_mesh(rng, 257, 64, big_ends=True)
    mats = rng.integers(1, 255, len(t)).astype(np.int32)
    want = check(ctx, v, t, 6, mats)
    assert (want[:, 3] == mats[-1]).sum() > 64 and (want[:, 3] == mats[0]).sum() > 64


# ---- 4. the grid-spanning triangle -------------------------------------------------------------------------------------------
def test_depth9_oblique_triangle(ctx):
    v, t = mm.oblique_triangle()
    stats = {}
    want = mm.voxelize(v, t, 9, stats=stats)
    assert (stats["tiles"], stats["kept"], stats["tests"], len(want)) == (262144, 4409, 2257408, 264697)
    got = ctx.voxelize_triangles(v, t, 9)
    assert np.array_equal(got, want)


# ---- 5. the edit form --------------------------------------------------------------------------------------------------------
def stamp_mesh(depth, rng):
    """A UV sphere, a torus and a grid-crossing triangle fitted into a grid of side 2^depth, materials inside a scene's table."""
    n = 1 << depth
    sv, st = mm.uv_sphere((n * 0.5, n * 0.55, n * 0.45), n * 0.3, 9, 12)
    tv, tt = mm.torus((n * 0.5, n * 0.4, n * 0.6), n * 0.32, n * 0.09, 14, 7)
    big = np.array([[-1.0, n * 0.2, n * 0.1], [n + 1.0, n * 0.7, n * 0.3], [n * 0.4, n + 1.0, n * 0.9]], np.float32)
    v = np.concatenate([sv, tv, big])
    t = np.concatenate([st, tt + len(sv), [[len(sv) + len(tv) + k for k in range(3)]]]).astype(np.uint32)
    return host.mesh_quantize(v), t, rng.integers(1, 21, len(t)).astype(np.int32)


def edit_cases(ctx, cells, depth, V, v, t, mats, tag):
    """Every op: the edit form against expected bytes and against the two-call composition; returns the SET result."""
    B = mm.voxelize(v, t, depth, mats)
    assert len(B) > 0 and 0 < np.isin(mm.morton(B[:, :3]), mm.morton(V[:, :3])).sum() < len(B)
    out = None
    for op in OPS:
        want_vox = apply_op(V, op, B, 0)
        built = built_cells(ctx, want_vox, depth)
        n_want = len(built) // 16
        room = max(len(cells) // 16, n_want) + 8
        vbo, counter = bind_cells(ctx, cells, room)
        n = ctx.octree_edit_triangles(op, v, t, mats)
        got = vbo.read(np.uint32)
        assert n == n_want and int(counter.read(np.uint32)[0]) == n, (tag, op)
        assert np.array_equal(got, padded(built, 64 * room)), (tag, op)
        vbo, counter = bind_cells(ctx, cells, room)
        assert ctx.octree_edit_voxels(op, ctx.voxelize_triangles(v, t, depth, mats)) == n
        assert np.array_equal(vbo.read(np.uint32), got), (tag, op)
        if op == rt.REGION_SET:
            out = got
    return out


def test_edit_triangles_on_config2_then_render(oracle):
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    v, t, mats = stamp_mesh(depth, np.random.default_rng(2))
    cam = host.camera_reference_pose(96, 64, 2, 3)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        edit_cases(ctx, cells, depth, V, v, t, mats, "config2")
        del vbos
    finally:
        ctx.close()
    room = 8 ** depth // 7 + 2                                  # no depth-6 tree has more cells
    r = rt.Renderer(host.Scene({**scene.blobs, 0: padded(cells, 64 * room)}), cam)
    try:
        r.render()                                              # derived tables of the tree as it was
        r.ctx.octree_edit_triangles(rt.REGION_SET, v, t, mats)
        got = r.vbos[0].read(np.uint32)
        img = r.render()
    finally:
        r.close()
    ref = oracle.render(host.Scene({**scene.blobs, 0: got}), cam, threads=4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


def test_edit_triangles_on_a_hand_built_tree_then_render(oracle):
    depth = 4
    vox = np.concatenate([block((0, 0, 0), (15, 2, 15), 3), block((4, 3, 4), (11, 10, 11), 5), [[15, 15, 15, 7]]]).astype(np.int32)
    v, t, mats = stamp_mesh(depth, np.random.default_rng(4))
    base = host.Scene.config(2)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    ctx = rt.Context(0)
    try:
        vbo, counter, V = bind_tree(ctx, vox, depth)
        cells = vbo.read(np.uint32)
        got = edit_cases(ctx, cells, depth, V, v, t, mats, "hand")
    finally:
        ctx.close()
    ints = np.array([depth, base.max_iter, base.cell_count], np.int32)
    scene = host.Scene({**base.blobs, 0: got, 7: ints})
    r = rt.Renderer(scene, cam)
    try:
        img = r.render()
    finally:
        r.close()
    ref = oracle.render(scene, cam, threads=4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


# ---- 6. errors leave every byte as it was ------------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    nc, nv = ctypes.c_uint32(0), ctypes.c_size_t(0)
    v = np.array([[U, U, U], [9 * U, 3 * U, 2 * U], [4 * U, 8 * U, 6 * U]], np.int32)
    t = np.array([[0, 1, 2]], np.uint32)
    ok, keep = rt._mesh(v, t, None, 0)
    ctx = rt.Context(0)
    try:
        # unbound slots: the edit form only
        for bound in ((), (0,), (7,)):
            for s in bound:
                b = rt.VertexBufferObject(ctx, cells if s == 0 else np.array([depth, 64, 128], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, b)
            assert L.tdt_octree_edit_triangles(ctx.h, 0, ctypes.byref(ok), ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        assert len(ctx.voxelize_triangles(v, t, 4)) > 0         # needs no tree
        vbos = rt.upload_scene(ctx, scene)
        counter = rt.VertexBufferObject(ctx, np.array([777], np.uint32))
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)

        def unchanged():
            return np.array_equal(vbos[0].read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 777

        far = v.copy()
        far[1, 2] = rt.MESH_COORD_MAX + 1
        neg = v.copy()
        neg[2, 0] = -rt.MESH_COORD_MAX - 1
        bad_t = np.array([[0, 1, 3]], np.uint32)
        E, X = ctx.octree_edit_triangles, ctx.voxelize_triangles
        cases = [lambda: E(0, v, bad_t), lambda: X(v, bad_t, 4), lambda: E(0, far, t), lambda: X(far, t, 4), lambda: X(neg, t, 4),
                 lambda: E(0, v, t, [0]), lambda: E(0, v, t, [255]), lambda: X(v, t, 4, [0]), lambda: X(v, t, 4, [255]),
                 lambda: E(0, v, t, None, 254), lambda: E(0, v, t, None, -1), lambda: X(v, t, 4, None, 254),
                 lambda: X(v, t, 0), lambda: X(v, t, 11), lambda: E(4, v, t), lambda: E(-1, v, t), lambda: E(rt.REGION_CLEAR, v, t, [0])]
        for i, f in enumerate(cases):
            with pytest.raises(rt.TdtError) as e:
                f()
            assert e.value.code == rt.ERR_INVALID_VALUE and unchanged(), i
        with pytest.raises(rt.TdtError, match="triangle 0"):
            E(0, v, bad_t)
        nomesh = rt.Mesh(None, None, None, 3, 1, 0, 0)          # counts above 0 with NULL arrays
        for rc in (L.tdt_octree_edit_triangles(ctx.h, 0, None, ctypes.byref(nc)),
                   L.tdt_octree_edit_triangles(ctx.h, 0, ctypes.byref(nomesh), ctypes.byref(nc)),
                   L.tdt_voxelize_triangles(ctx.h, None, 4, None, 0, ctypes.byref(nv)),
                   L.tdt_voxelize_triangles(ctx.h, ctypes.byref(nomesh), 4, None, 0, ctypes.byref(nv)),
                   L.tdt_voxelize_triangles(ctx.h, ctypes.byref(ok), 4, None, 0, None)):
            assert rc == rt.ERR_INVALID_VALUE and unchanged()
        # the level-1 cap, found on the host: whole-grid diagonals at depth 10 are 128^3 = 2^21 tiles each
        seg = np.array([[0, 0, 0], [1024 * U, 1024 * U, 1024 * U], [0, 0, 0]], np.int32)
        t33 = np.tile(np.array([[0, 1, 2]], np.uint32), (33, 1))
        assert sum(mm.tile_candidates(seg[i], 10) for i in t33) > rt.REGION_BRUSH_CAP
        with pytest.raises(rt.TdtError, match=str(33 << 21)) as e:
            X(seg, t33, 10)
        assert e.value.code == rt.ERR_INVALID_VALUE
        vb10, counter10, _ = bind_tree(ctx, np.array([[1, 1, 1, 1], [1000, 2, 3, 4]], np.int32), 10)
        before = vb10.read(np.uint32)
        with pytest.raises(rt.TdtError, match=str(33 << 21)) as e:
            E(rt.REGION_SET, seg, t33)
        assert e.value.code == rt.ERR_INVALID_VALUE and np.array_equal(vb10.read(np.uint32), before)
        assert int(counter10.read(np.uint32)[0]) == 12345
        # extract form: NULL counts only; a capacity below the count: the count, nothing written
        want = mm.voxelize(v, t, 4)
        assert L.tdt_voxelize_triangles(ctx.h, ctypes.byref(ok), 4, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == len(want)
        out = np.zeros((len(want), 4), np.int32)
        nv = ctypes.c_size_t(0)
        assert L.tdt_voxelize_triangles(ctx.h, ctypes.byref(ok), 4, out.ctypes.data, len(want) - 1, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
        assert nv.value == len(want) and not out.any()
        assert L.tdt_voxelize_triangles(ctx.h, ctypes.byref(ok), 4, out.ctypes.data, len(want), ctypes.byref(nv)) == rt.OK
        assert np.array_equal(out, want)
        # an empty mesh, and a mesh wholly off the grid: an empty list
        assert X(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), 4).shape == (0, 4)
        assert X(v - 40 * U, t, 4).shape == (0, 4)
        # a misfit: a buffer one cell too small reports the count it needs and keeps its bytes
        vbo, counter2, V1 = bind_tree(ctx, np.array([[3, 3, 3, 5]], np.int32), 4)
        chain = vbo.read(np.uint32)
        built = built_cells(ctx, apply_op(V1, rt.REGION_SET, want, 0), 4)
        need = len(built) // 16
        assert need > len(chain) // 16
        vbo, counter2 = bind_cells(ctx, chain, need - 1)
        with pytest.raises(rt.TdtError) as e:
            E(rt.REGION_SET, v, t)
        assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
        assert np.array_equal(vbo.read(np.uint32), padded(chain, 64 * (need - 1))) and int(counter2.read(np.uint32)[0]) == 12345
        vbo, counter2 = bind_cells(ctx, chain, need)
        assert E(rt.REGION_SET, v, t) == need and np.array_equal(vbo.read(np.uint32), built)
        # an empty mesh, edit form: an empty brush, i.e. the tree's compacted bytes
        vbo, counter2 = bind_cells(ctx, chain, need)
        assert E(rt.REGION_SET, np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32)) == len(chain) // 16
        assert np.array_equal(vbo.read(np.uint32), padded(chain, 64 * need))
        del keep
    finally:
        ctx.close()


# ---- 7. ordering -------------------------------------------------------------------------------------------------------------
def test_edit_dispatched_just_before_is_included(oracle):
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 34000, np.uint32)])
    d = distinct_deltas(np.random.default_rng(21), 200, depth, scene.blobs[0])
    d[:, 3], d[:, 4] = 2.0, 4.0
    edited, _ = oracle_py.oracle_octree_update(oracle, scene, d, used, (len(d), 1, 1))
    v, t, mats = stamp_mesh(depth, np.random.default_rng(8))
    r, upd, counter = edit_setup(scene, used, d)
    try:
        ctx2 = rt.Context(0)
        try:
            bind_cells(ctx2, edited, len(edited) // 16)
            v7 = rt.VertexBufferObject(ctx2, scene.blobs[7])
            ctx2.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, v7)
            V = ctx2.octree_extract()
            want_vox = apply_op(V, rt.REGION_FILL, mm.voxelize(v, t, depth, mats), 0)
            want, n_want = expected_bytes(ctx2, want_vox, depth, scene.blobs[0].nbytes)
        finally:
            ctx2.close()
        upd.dispatch_compute(len(d), 1, 1)                 # no finish
        n = r.ctx.octree_edit_triangles(rt.REGION_FILL, v, t, mats)
        assert n == n_want and np.array_equal(r.vbos[0].read(np.uint32), want)
        assert int(counter.read(np.uint32)[0]) == n
    finally:
        r.close()


# ---- 8. multi-device ---------------------------------------------------------------------------------------------------------
def test_multi_device_context():
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    scene.blobs[0] = padded(cells, 64 * (8 ** depth // 7 + 2))
    cam = host.camera_reference_pose(96, 64, 2, 3)
    v, t, mats = stamp_mesh(depth, np.random.default_rng(9))
    outs = []
    for devices in (None, [0, 0]):                             # two members on one device: every replica path, on any machine
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            lst = r.ctx.voxelize_triangles(v, t, depth, mats)
            before = r.vbos[0].read(np.uint32)
            with pytest.raises(rt.TdtError):
                r.ctx.octree_edit_triangles(rt.REGION_SET, v, t, np.zeros(len(t), np.int32))
            assert np.array_equal(r.vbos[0].read(np.uint32), before)
            n = r.ctx.octree_edit_triangles(rt.REGION_SET, v, t, mats)
            outs.append((n, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), lst))
        finally:
            r.close()
    (n1, c1, img1, v1, l1), (n2, c2, img2, v2, l2) = outs
    assert n1 == n2 and np.array_equal(c1, c2) and np.array_equal(v1, v2) and np.array_equal(l1, l2)
    assert np.array_equal(l1, mm.voxelize(v, t, depth, mats))
    assert (img1.view(np.uint32) == img2.view(np.uint32)).all()


# ---- 9. the demo -------------------------------------------------------------------------------------------------------------
CUBE_PLY = """ply
format ascii 1.0
comment a unit cube as six quads
element vertex 8
property float x
property float y
property float z
element face 6
property list uchar int vertex_indices
end_header
0 0 0
1 0 0
1 1 0
0 1 0
0 0 1
1 0 1
1 1 1
0 1 1
4 0 1 2 3
4 4 5 6 7
4 0 1 5 4
4 1 2 6 5
4 2 3 7 6
4 3 0 4 7
"""


def test_demo_mesh_equals_the_model_and_the_oracle(oracle, tmp_path):
    exe = build.build_demo()
    ply = tmp_path / "cube.ply"
    ply.write_text(CUBE_PLY)
    out = str(tmp_path / "frame.pfm")
    w, h = 96, 64
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    cam = host.camera_reference_pose(w, h, 2, 3)
    lo, hi = (20, 30, 10), (43, 49, 33)
    mesh = host.PlyMesh(ply.read_bytes())
    scale, off = host.mesh_fit(mesh.vertices, lo, hi)
    q = host.mesh_quantize(mesh.vertices, scale, off)
    B = mm.voxelize(q, mesh.triangles, depth, None, 6)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        want_vox = apply_op(ctx.octree_extract(), rt.REGION_SET, B, 0)
        built = built_cells(ctx, want_vox, depth)
        del vbos
    finally:
        ctx.close()
    n = len(built) // 16
    room = max(len(cells) // 16, n)
    p = subprocess.run([exe, "--config", "2", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "3", "--cells", str(room), "--mesh", str(ply),
                        "--material", "6", "--box", ",".join(str(c) for c in lo + hi), "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"mesh triangles 12 voxels {len(B)} op set cells {n}\b", p.stdout), p.stdout
    ref = oracle.render(host.Scene({**scene.blobs, 0: padded(built, 64 * room)}), cam, threads=8)
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF4"
        fw, fh = map(int, f.readline().split())
        f.readline()
        img = np.frombuffer(f.read(), "<f4").reshape(fh, fw, 4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()
