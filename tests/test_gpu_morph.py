"""Voxel morphology (tdt_octree_morph / tdt_octree_extract_morph): the extracted list must equal the numpy model bit for bit,
and an edit must leave in the bound cells buffer exactly the builder's tree of the model's voxel list followed by zeros — on
the library's scenes (merged LEAFs, shared cells, an edit session with dead cells), on hand-built trees that pin the grid
faces, the inherit rule and the empty result, after a queued edit, on a multi-device context and through the demo."""
import ctypes
import itertools
import re
import subprocess

import numpy as np
import pytest

import morph_model as mm
import oracle_py
from octree_util import distinct_deltas, edit_setup
from test_gpu_connect import bind_tree, block, hand_trees
from test_gpu_region_edit import bind_cells, built_cells, expected_bytes, padded, scene_by_name, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
OPS = (rt.MORPH_DILATE, rt.MORPH_ERODE, rt.MORPH_OPEN, rt.MORPH_CLOSE, rt.MORPH_SHELL)
FULL_TREE_CELLS_DEPTH6 = sum(8 ** l for l in range(6))      # no depth-6 tree (config 2) has more cells: any result fits


def check_case(ctx, cells, V, depth, cache, tag, **kw):
    """extract_morph and octree_morph of one case against the model, on a fresh copy of `cells` with room for the result."""
    want_vox = mm.morph(V, depth, cache=cache, **kw)
    built = built_cells(ctx, want_vox, depth)
    n_want = len(built) // 16
    room = max(len(cells) // 16, n_want) + 8
    vbo, counter = bind_cells(ctx, cells, room)
    got = ctx.octree_extract_morph(**kw)
    assert got.shape == want_vox.shape and np.array_equal(got, want_vox), tag
    assert np.array_equal(vbo.read(np.uint32), padded(cells, 64 * room)) and int(counter.read(np.uint32)[0]) == 12345, tag
    n = ctx.octree_morph(**kw)
    assert n == n_want, tag
    assert int(counter.read(np.uint32)[0]) == n, tag
    assert np.array_equal(vbo.read(np.uint32), padded(built, 64 * room)), tag
    return want_vox


# ---- 1. every op on the library's scenes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["config1", "config2", "config3", "config5", "monument", "session"])
def test_morph_equals_the_numpy_model(name):
    scene = scene_by_name(name)
    depth, n = scene.max_depth, 1 << scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    radii = (1, 2) if name in ("config3", "config5") else (1, 3)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        assert len(V)
        cache = {}
        cases = [dict(op=op, connectivity=conn, radius=r) for op, conn, r in itertools.product(OPS, (6, 26), radii)]
        c = V[len(V) // 2, :3].astype(int)
        cases += [dict(op=rt.MORPH_DILATE, connectivity=6, radius=1, material=7),
                  dict(op=rt.MORPH_ERODE, connectivity=26, radius=1, border=1),
                  dict(op=rt.MORPH_CLOSE, connectivity=6, radius=1, regions=[rt.box(c - n // 8, c + n // 16), rt.sphere(c + n // 8, n // 6)])]
        sizes = set()
        for case in cases:
            sizes.add(len(check_case(ctx, cells, V, depth, cache, f"{name} {case}", **case)))
        assert len(sizes) > 4                                   # the cases are not all the same list
        del vbos
    finally:
        ctx.close()


# ---- 2. extract_morph changes nothing ------------------------------------------------------------------------------------
def test_extract_morph_leaves_the_tree_alone():
    scene = host.Scene.config(2)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    r = rt.Renderer(scene, cam)
    try:
        counter = rt.VertexBufferObject(r.ctx, np.array([4321], np.uint32))
        r.ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)
        before, cells = r.render(), r.vbos[0].read(np.uint32)
        V = r.ctx.octree_extract()
        for op, conn in itertools.product(OPS, (6, 26)):
            got = r.ctx.octree_extract_morph(op, 2, conn, material=5 if op == rt.MORPH_CLOSE else None)
            assert np.array_equal(got, mm.morph(V, scene.max_depth, op, 2, conn, 5 if op == rt.MORPH_CLOSE else None)), (op, conn)
            assert np.array_equal(r.vbos[0].read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 4321
        # NULL: the count only; a capacity below it: the count, nothing written
        L = rt.lib()
        m = rt.Morph(rt.MORPH_SHELL, 26, 1, -1, 0, 0)
        want = mm.morph(V, scene.max_depth, rt.MORPH_SHELL, 1, 26)
        nv = ctypes.c_size_t(0)
        assert L.tdt_octree_extract_morph(r.ctx.h, ctypes.byref(m), None, 0, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == len(want)
        out = np.zeros((len(want), 4), np.int32)
        nv = ctypes.c_size_t(0)
        assert L.tdt_octree_extract_morph(r.ctx.h, ctypes.byref(m), None, 0, out.ctypes.data, len(want) - 1, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
        assert nv.value == len(want) and not out.any()
        assert L.tdt_octree_extract_morph(r.ctx.h, ctypes.byref(m), None, 0, out.ctypes.data, len(want), ctypes.byref(nv)) == rt.OK
        assert np.array_equal(out, want)
        after = r.render()
        assert (before.view(np.uint32) == after.view(np.uint32)).all()
    finally:
        r.close()


# ---- 3. hand-built trees -------------------------------------------------------------------------------------------------
def run_hand(vox, depth, **kw):
    """(extracted list, cell count, cells words) of one morph on the builder's tree of vox, in a buffer just large enough for the
    tree and the result; all checked against the model."""
    ctx = rt.Context(0)
    try:
        vbo, counter, V = bind_tree(ctx, vox, depth)
        want = mm.morph(V, depth, **kw)
        got = ctx.octree_extract_morph(**kw)
        assert np.array_equal(got, want), kw
        built = built_cells(ctx, want, depth)
        before = vbo.read(np.uint32)
        room = max(len(before), len(built)) // 16
        if room > len(before) // 16:
            vbo, counter = bind_cells(ctx, before, room)
        n = ctx.octree_morph(**kw)
        cells = vbo.read(np.uint32)
        assert n == len(built) // 16 and np.array_equal(cells, padded(built, 64 * room)) and int(counter.read(np.uint32)[0]) == n, kw
        assert np.array_equal(ctx.octree_extract(), want), kw
        return got, n, cells
    finally:
        ctx.close()


def test_hand_checkerboard_close_fills_the_block():
    vox, depth = hand_trees()["checkerboard"][:2]
    got, n, cells = run_hand(vox, depth, op=rt.MORPH_CLOSE, radius=1, connectivity=6)
    assert np.array_equal(got, sort_vox(block((0, 0, 0), (7, 7, 7), 4)))


def test_hand_solid_block_erode_and_shell():
    vox, depth = hand_trees()["solid_64"][:2]                    # the input is one merged LEAF per root node
    got, n, _ = run_hand(vox, depth, op=rt.MORPH_SHELL, radius=1, connectivity=26, border=1)
    assert len(got) == 0 and n == 1
    got, _, _ = run_hand(vox, depth, op=rt.MORPH_SHELL, radius=1, connectivity=6, border=0)
    assert len(got) == 64 ** 3 - 62 ** 3 and ((got[:, :3] == 0) | (got[:, :3] == 63)).any(1).all()
    got, _, _ = run_hand(vox, depth, op=rt.MORPH_ERODE, radius=3, connectivity=26, border=0)
    assert np.array_equal(got, sort_vox(block((3, 3, 3), (60, 60, 60), 9)))
    got, _, _ = run_hand(vox, depth, op=rt.MORPH_ERODE, radius=2, connectivity=6, border=1)
    assert len(got) == 64 ** 3


def test_hand_depth10_corners_dilate_clips_at_the_grid():
    vox, depth = hand_trees()["depth10_corners"][:2]
    got, _, _ = run_hand(vox, depth, op=rt.MORPH_DILATE, radius=2, connectivity=26)
    assert (got[:, :3] >= 0).all() and (got[:, :3] < 1024).all()
    # (0,0,0) and (1,1,1) grow into the clipped cube [0, 3]^3; nothing appears across a grid face
    assert (got[:, :3].max(1) <= 3).sum() == 4 ** 3
    far = got[(got[:, :3] >= 1021).all(1)]
    assert len(far) == 3 * 3 * 3 and (far[:, 3] == 2).all()


def test_hand_serpentine_open_removes_everything():
    vox, depth = hand_trees()["serpentine"][:2]
    got, n, cells = run_hand(vox, depth, op=rt.MORPH_OPEN, radius=1, connectivity=6)
    assert len(got) == 0 and n == 1 and not cells.any()


def test_hand_inherit_rule():
    # an empty voxel flanked by material 3 at -x (d = (-1, 0, 0), t = 4) and material 8 at +x (t = 22): the lower t wins
    vox = np.array([[3, 4, 4, 4], [5, 4, 4, 9]], np.int32)
    got, _, _ = run_hand(vox, 3, op=rt.MORPH_DILATE, radius=1, connectivity=6)
    assert got[(got[:, :3] == (4, 4, 4)).all(1), 3].tolist() == [4]
    got, _, _ = run_hand(vox, 3, op=rt.MORPH_DILATE, radius=1, connectivity=26)
    assert got[(got[:, :3] == (4, 5, 4)).all(1), 3].tolist() == [4] and got[(got[:, :3] == (6, 4, 4)).all(1), 3].tolist() == [9]
    got, _, _ = run_hand(vox, 3, op=rt.MORPH_DILATE, radius=1, connectivity=26, material=0)
    assert sorted(got[:, 3].tolist()) == [1] * (len(got) - 2) + [4, 9]


# ---- 4. ordering: directly after a queued edit ---------------------------------------------------------------------------
def test_morph_after_a_queued_edit_dispatch(oracle):
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = padded(np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), 64 * FULL_TREE_CELLS_DEPTH6)
    d = distinct_deltas(np.random.default_rng(23), 200, depth, scene.blobs[0])
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
            want_vox = mm.morph(V, depth, rt.MORPH_DILATE, 1, 26)
            want, n_want = expected_bytes(ctx2, want_vox, depth, scene.blobs[0].nbytes)
        finally:
            ctx2.close()
        upd.dispatch_compute(len(d), 1, 1)                 # no finish
        n = r.ctx.octree_morph(rt.MORPH_DILATE, 1, 26)
        assert n == n_want and np.array_equal(r.vbos[0].read(np.uint32), want)
        assert int(counter.read(np.uint32)[0]) == n
    finally:
        r.close()


# ---- 5. errors leave every byte as it was --------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    nc, nv = ctypes.c_uint32(0), ctypes.c_size_t(0)
    ok = rt.Morph(rt.MORPH_ERODE, 6, 1, -1, 0, 0)
    ctx = rt.Context(0)
    try:
        for bound in ((), (0,), (7,)):
            for s in bound:
                v = rt.VertexBufferObject(ctx, cells if s == 0 else np.array([depth, 64, 128], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, v)
            assert L.tdt_octree_morph(ctx.h, ctypes.byref(ok), None, 0, ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract_morph(ctx.h, ctypes.byref(ok), None, 0, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        vbos = rt.upload_scene(ctx, scene)
        counter = rt.VertexBufferObject(ctx, np.array([777], np.uint32))
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)

        def unchanged():
            return np.array_equal(vbos[0].read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 777

        bad_shape = rt.box((0, 0, 0), (1, 1, 1))
        bad_shape.shape = 7
        M, X = ctx.octree_morph, ctx.octree_extract_morph
        cases = [lambda: M(5), lambda: M(-1), lambda: M(rt.MORPH_ERODE, connectivity=18), lambda: M(rt.MORPH_ERODE, connectivity=0),
                 lambda: M(rt.MORPH_ERODE, radius=0), lambda: M(rt.MORPH_ERODE, radius=65), lambda: M(rt.MORPH_ERODE, radius=-3),
                 lambda: M(rt.MORPH_DILATE, material=254), lambda: M(rt.MORPH_DILATE, material=-2), lambda: M(rt.MORPH_ERODE, border=2),
                 lambda: M(rt.MORPH_ERODE, border=-1), lambda: M(rt.MORPH_ERODE, regions=bad_shape),
                 lambda: M(rt.MORPH_ERODE, regions=rt.sphere((1, 1, 1), -1)),
                 lambda: X(7), lambda: X(rt.MORPH_SHELL, connectivity=8), lambda: X(rt.MORPH_SHELL, radius=0), lambda: X(rt.MORPH_CLOSE, material=300),
                 lambda: X(rt.MORPH_SHELL, border=3), lambda: X(rt.MORPH_SHELL, regions=bad_shape)]
        for i, f in enumerate(cases):
            with pytest.raises(rt.TdtError) as e:
                f()
            assert e.value.code == rt.ERR_INVALID_VALUE and unchanged(), i
        for rc in (L.tdt_octree_morph(ctx.h, None, None, 0, ctypes.byref(nc)),
                   L.tdt_octree_morph(ctx.h, ctypes.byref(ok), None, 1, ctypes.byref(nc)),
                   L.tdt_octree_extract_morph(ctx.h, ctypes.byref(ok), None, 2, None, 0, ctypes.byref(nv)),
                   L.tdt_octree_extract_morph(ctx.h, None, None, 0, None, 0, ctypes.byref(nv))):
            assert rc == rt.ERR_INVALID_VALUE and unchanged()
        # a LEAF value >= 254 cannot be rebuilt: both forms refuse it
        bad = cells.copy()
        bad[2 * int(np.flatnonzero(cells[1::2] == 2)[0])] = 254
        vbo, counter3 = bind_cells(ctx, bad, len(bad) // 16 + 64)
        for f in (lambda: ctx.octree_morph(rt.MORPH_ERODE), lambda: ctx.octree_extract_morph(rt.MORPH_ERODE)):
            with pytest.raises(rt.TdtError) as e:
                f()
            assert e.value.code == rt.ERR_INVALID_VALUE
            assert np.array_equal(vbo.read(np.uint32), padded(bad, vbo.nbytes)) and int(counter3.read(np.uint32)[0]) == 12345
        # a DILATE that does not fit (one voxel: a chain of cells; its 26-neighbourhood straddles the octants): the cell count it
        # needs, nothing written; the same call on a buffer of that size then succeeds
        vbo, counter2, V1 = bind_tree(ctx, np.array([[32, 32, 32, 5]], np.int32), 6)
        chain = vbo.read(np.uint32)
        built = built_cells(ctx, mm.morph(V1, 6, rt.MORPH_DILATE, 1, 26), 6)
        need = len(built) // 16
        assert need > len(chain) // 16
        with pytest.raises(rt.TdtError) as e:
            ctx.octree_morph(rt.MORPH_DILATE, 1, 26)
        assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
        assert np.array_equal(vbo.read(np.uint32), chain) and int(counter2.read(np.uint32)[0]) == 12345
        vbo, counter2 = bind_cells(ctx, chain, need)
        assert ctx.octree_morph(rt.MORPH_DILATE, 1, 26) == need
        assert np.array_equal(vbo.read(np.uint32), built) and int(counter2.read(np.uint32)[0]) == need
        # Python-side checks raise before the call
        with pytest.raises(ValueError):
            ctx.octree_morph(rt.MORPH_ERODE, radius=2**32 + 1)
        del vbos
    finally:
        ctx.close()


# ---- 6. the frame after a morph -------------------------------------------------------------------------------------------
def test_frame_after_morph_equals_a_fresh_upload_of_the_model_tree():
    scene = host.Scene.config(3)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    cam = host.camera_reference_pose(128, 96, 2, 4)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        want_vox = mm.morph(ctx.octree_extract(), depth, rt.MORPH_ERODE, 2, 6)
        built = built_cells(ctx, want_vox, depth)
        del vbos
    finally:
        ctx.close()
    room = max(len(cells), len(built)) // 16 + 8             # an erosion moves faces off the merged blocks: it may need more cells
    r = rt.Renderer(host.Scene({**scene.blobs, 0: padded(cells, 64 * room)}), cam)
    try:
        r.render()                                          # the LDS image / tables / bricks of the original tree exist
        assert r.ctx.octree_morph(rt.MORPH_ERODE, 2, 6) == len(built) // 16
        assert np.array_equal(r.vbos[0].read(np.uint32), padded(built, 64 * room))
        img = r.render()
    finally:
        r.close()
    fresh = rt.Renderer(host.Scene({**scene.blobs, 0: padded(built, 64 * room)}), cam)
    try:
        ref = fresh.render()
    finally:
        fresh.close()
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


# ---- 7. multi-device -----------------------------------------------------------------------------------------------------
def test_multi_device_morph_renders_like_a_single_device(oracle):
    scene = host.Scene.config(2)
    scene.blobs[0] = padded(np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), 64 * FULL_TREE_CELLS_DEPTH6)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            V = r.ctx.octree_extract()
            c = V[len(V) // 2, :3].astype(int)
            preview = r.ctx.octree_extract_morph(rt.MORPH_CLOSE, 1, 26)
            n = r.ctx.octree_morph(rt.MORPH_CLOSE, 1, 26)
            n += r.ctx.octree_morph(rt.MORPH_SHELL, 1, 6, regions=[rt.sphere(c, 12)])
            outs.append((n, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), preview))
        finally:
            r.close()
    (n1, c1, img1, v1, p1), (n2, c2, img2, v2, p2) = outs
    assert n1 == n2 and np.array_equal(c1, c2) and np.array_equal(v1, v2) and np.array_equal(p1, p2)
    assert (img1.view(np.uint32) == img2.view(np.uint32)).all()
    assert (img1.view(np.uint32) == oracle.render(host.Scene({**scene.blobs, 0: c1}), cam, threads=4).view(np.uint32)).all()


# ---- 8. the demo ---------------------------------------------------------------------------------------------------------
def test_demo_morph_shell_equals_the_oracle(oracle, tmp_path):
    exe = build.build_demo()
    out = str(tmp_path / "frame.pfm")
    w, h = 128, 96
    scene = host.Scene.config(3)
    depth = scene.max_depth
    cam = host.camera_reference_pose(w, h, 2, 6)
    room = len(np.asarray(scene.blobs[0]).view(np.uint32)) // 16          # the demo uploads the scene's cells buffer as it is
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        want_vox = mm.morph(V, depth, rt.MORPH_SHELL, 1, 6)
        built = built_cells(ctx, want_vox, depth)
        del vbos
    finally:
        ctx.close()
    n = len(built) // 16
    assert 0 < len(want_vox) < len(V)
    room = max(room, n)                                     # hollowing splits merged LEAFs: --cells gives the buffer the room
    p = subprocess.run([exe, "--config", "3", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "6", "--cells", str(room), "--morph", "shell:1",
                        "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"morph shell:1 conn 6 cells {n}\b", p.stdout), p.stdout
    ref = oracle.render(host.Scene({**scene.blobs, 0: padded(built, 64 * room)}), cam, threads=8)
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF4"
        fw, fh = map(int, f.readline().split())
        f.readline()
        img = np.frombuffer(f.read(), "<f4").reshape(fh, fw, 4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()
