"""Connected components (tdt_octree_components / tdt_octree_edit_connected / tdt_octree_extract_connected): labels and the
component table must equal the numpy model bit for bit, and an edit must leave in the bound cells buffer exactly the
builder's tree of the model's voxel list followed by zeros — on built trees with merged LEAFs, shared cells, edit sessions
with dead cells and hand-built trees that stress the union-find and the per-component reductions."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import connect_model as cm
import oracle_py
from octree_util import distinct_deltas, edit_setup
from test_gpu_region_edit import bind_cells, built_cells, expected_bytes, morton, padded, scene_by_name, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
KINDS = [(6, rt.MATCH_ANY), (26, rt.MATCH_ANY), (6, rt.MATCH_MATERIAL), (26, rt.MATCH_MATERIAL)]
# (components at 6 / ANY, at 26 / ANY, at 6 / MATERIAL): counted on the CPU with an independent labelling
SCENE_COUNTS = {"config3": (20, 20, 265), "config5": (206, 18, 812)}


def bind_tree(ctx, vox, depth, room=0):
    """The builder's tree of a voxel list bound to slots 0 (with `room` extra cells) and 7; returns (cells vbo, counter, V)."""
    vox = sort_vox(vox)
    built = built_cells(ctx, vox, depth)
    vbo, counter = bind_cells(ctx, built, len(built) // 16 + room)
    ints = rt.VertexBufferObject(ctx, np.array([depth, 64, 1 << depth], np.int32))
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
    ctx._keep = (vbo, counter, ints)                     # the buffers live as long as the context uses them
    return vbo, counter, vox


def check_components(ctx, V, depth, tag):
    """Every connectivity and match rule against the model; returns the component counts."""
    counts = {}
    for conn, match in KINDS:
        labels, tab = ctx.octree_components(conn, match)
        want_l, want_t = cm.components(V, depth, conn, match)
        assert np.array_equal(labels, want_l), (tag, conn, match)
        assert tab.tobytes() == want_t.tobytes(), (tag, conn, match)
        counts[(conn, match)] = len(tab)
    return counts


# ---- 1. labels and table on the library's scenes -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["config1", "config2", "config3", "config5", "monument", "session"])
def test_components_equal_the_numpy_model(name):
    scene = scene_by_name(name)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        counts = check_components(ctx, V, scene.max_depth, name)
        if name in SCENE_COUNTS:
            want = SCENE_COUNTS[name]
            assert (counts[(6, rt.MATCH_ANY)], counts[(26, rt.MATCH_ANY)], counts[(6, rt.MATCH_MATERIAL)]) == want
        del vbos
    finally:
        ctx.close()


# ---- 2. hand-built trees -------------------------------------------------------------------------------------------------
def block(lo, hi, m=1):
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([g, np.full((len(g), 1), m)], 1).astype(np.int32)


def serpentine(n):
    """A one-voxel-wide path through an n^3 grid: rows along x on even y of even z, joined at alternating ends, layers joined at
    alternating corners."""
    pts = []
    for li, z in enumerate(range(0, n, 2)):
        ys = list(range(0, n, 2))
        if li % 2:
            ys = ys[::-1]
        for ri, y in enumerate(ys):
            xs = range(n) if (li * len(ys) + ri) % 2 == 0 else range(n - 1, -1, -1)
            pts += [(x, y, z) for x in xs]
            if ri + 1 < len(ys):
                pts.append((pts[-1][0], y + (1 if ys[ri + 1] > y else -1), z))
        if z + 2 < n:
            pts.append((pts[-1][0], pts[-1][1], z + 1))
    p = np.array(pts, np.int32)
    assert len(np.unique(p, axis=0)) == len(p)
    return np.concatenate([p, np.full((len(p), 1), 3, np.int32)], 1)


def hand_trees():
    cube = block((0, 0, 0), (1, 1, 1), 2)
    chk = block((0, 0, 0), (7, 7, 7), 4)
    chk = chk[(chk[:, :3].sum(1) % 2) == 0]
    N10 = 1 << 10
    return {                       # name: (voxels, depth, components at 6 / ANY, at 26 / ANY)
        "edge": (np.concatenate([cube, block((2, 2, 0), (3, 3, 1), 2)]), 3, 2, 1),
        "corner": (np.concatenate([cube, block((2, 2, 2), (3, 3, 3), 5)]), 3, 2, 1),
        "checkerboard": (chk, 3, len(chk), 1),
        "serpentine": (serpentine(64), 6, 1, 1),
        "opposite_faces": (np.array([[0, 5, 5, 1], [15, 5, 5, 1], [5, 0, 5, 1], [5, 15, 5, 1], [0, 0, 0, 1], [15, 15, 15, 1]], np.int32), 4,
                           6, 6),
        "leaf_and_voxel": (np.concatenate([block((0, 0, 0), (7, 7, 7), 6), [[8, 3, 3, 6], [8, 8, 8, 7]]]), 4, 2, 1),
        "solid_64": (block((0, 0, 0), (63, 63, 63), 9), 6, 1, 1),
        "depth10_corners": (np.array([[0, 0, 0, 1], [1, 1, 1, 1], [N10 - 1, N10 - 1, N10 - 1, 2], [N10 - 1, N10 - 1, N10 - 2, 2],
                                      [N10 - 1, 0, 0, 3], [0, N10 - 1, N10 - 1, 3]], np.int32), 10, 5, 4),
    }


@pytest.mark.parametrize("name", list(hand_trees()))
def test_hand_built_trees(name):
    vox, depth, want6, want26 = hand_trees()[name]
    ctx = rt.Context(0)
    try:
        _, _, V = bind_tree(ctx, vox, depth)
        assert np.array_equal(ctx.octree_extract(), V)
        counts = check_components(ctx, V, depth, name)
        assert (counts[(6, rt.MATCH_ANY)], counts[(26, rt.MATCH_ANY)]) == (want6, want26), counts
        if name == "solid_64":
            _, tab = ctx.octree_components(26, rt.MATCH_ANY)
            assert tab["voxels"][0] == 64 ** 3 and list(tab["lo"][0]) == [0] * 3 and list(tab["hi"][0]) == [63] * 3
    finally:
        ctx.close()


# ---- 3. every selection form and op --------------------------------------------------------------------------------------
def selection_cases(V, depth):
    """Seeds (on the second-largest component, on air and off the grid), a size window, regions touching; each with invert."""
    n = 1 << depth
    labels, tab = cm.components(V, depth, 6, rt.MATCH_ANY)
    big = np.argsort(-tab["voxels"].astype(np.int64), kind="stable")
    c = int(big[1] if len(big) > 1 else big[0])
    seed = V[tab["first"][c], :3]
    occupied = set(map(tuple, V[:, :3].tolist()))
    air = next(p for p in ((x, n - 1, n - 1) for x in range(n)) if p not in occupied)
    corner = V[tab["first"][int(big[-1])], :3]
    cases = []
    for invert in (False, True):
        cases += [dict(seeds=[seed, air, (-1, 2, 3)], invert=invert, connectivity=6, match=rt.MATCH_ANY),
                  dict(seeds=[seed], invert=invert, connectivity=26, match=rt.MATCH_MATERIAL),
                  dict(min_voxels=1, max_voxels=int(np.median(tab["voxels"])), invert=invert, connectivity=26, match=rt.MATCH_ANY),
                  dict(regions=[rt.box(corner - 1, corner + 1), rt.sphere(seed, 2)], invert=invert, connectivity=6,
                       match=rt.MATCH_MATERIAL)]
    return cases


@pytest.mark.parametrize("name", ["config2", "config3"])
def test_edit_connected_equals_the_numpy_model(name):
    scene = scene_by_name(name)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        for case in selection_cases(V, depth):
            sel = {k: v for k, v in case.items() if k not in ("connectivity", "match")}
            for op in (rt.REGION_PAINT, rt.REGION_CLEAR):
                want_vox = cm.edit(V, depth, op, 11, case["connectivity"], case["match"], **sel)
                built = built_cells(ctx, want_vox, depth)
                n_want = len(built) // 16
                room = max(len(cells) // 16, n_want) + 8
                vbo, counter = bind_cells(ctx, cells, room)
                tag = f"{name} op {op} {case}"
                assert np.array_equal(ctx.octree_extract_connected(**case), cm.extract(V, depth, case["connectivity"], case["match"], **sel)), tag
                n = ctx.octree_edit_connected(op, material=11, **case)
                assert n == n_want, tag
                assert int(counter.read(np.uint32)[0]) == n, tag
                assert np.array_equal(vbo.read(np.uint32), padded(built, 64 * room)), tag
                assert np.array_equal(ctx.octree_extract(), want_vox), tag
        del vbos
    finally:
        ctx.close()


def test_scene_stories_floating_parts_and_debris():
    ctx = rt.Context(0)
    try:
        scene = scene_by_name("config3")
        depth, n = scene.max_depth, 1 << scene.max_depth
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        ground = [rt.box((0, 0, 0), (n - 1, 12, n - 1))]
        want_vox = cm.edit(V, depth, rt.REGION_CLEAR, regions=ground, invert=True)
        assert len(want_vox) == 422581
        want, n_want = expected_bytes(ctx, want_vox, depth, cells_bytes(vbos[0]))
        assert ctx.octree_edit_connected(rt.REGION_CLEAR, regions=ground, invert=True) == n_want
        assert np.array_equal(vbos[0].read(np.uint32), want)
        assert np.array_equal(ctx.octree_extract(), want_vox)
        _, tab = ctx.octree_components()
        assert len(tab) == 1 and tab["voxels"][0] == 422581 and tab["lo"][0][1] == 12

        scene = scene_by_name("config5")
        depth = scene.max_depth
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        _, before = ctx.octree_components()
        small = before["voxels"] <= 8
        assert len(before) == 206 and small.sum() == 76
        want_vox = cm.edit(V, depth, rt.REGION_CLEAR, min_voxels=1, max_voxels=8)
        assert len(want_vox) == len(V) - int(before["voxels"][small].sum())
        want, n_want = expected_bytes(ctx, want_vox, depth, cells_bytes(vbos[0]))
        assert ctx.octree_edit_connected(rt.REGION_CLEAR, min_voxels=1, max_voxels=8) == n_want
        assert np.array_equal(vbos[0].read(np.uint32), want)
        _, after = ctx.octree_components()
        assert len(after) == 206 - 76 and np.array_equal(np.sort(after["voxels"]), np.sort(before["voxels"][~small]))
    finally:
        ctx.close()


def cells_bytes(vbo):
    return vbo.read(np.uint32).nbytes


# ---- 4. extract, clear, undo ---------------------------------------------------------------------------------------------
def test_extract_connected_clear_and_undo():
    scene = host.Scene.config(3)
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 4096, np.uint32)])
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        ctx.octree_compact()
        compacted = vbos[0].read(np.uint32)
        V = ctx.octree_extract()
        _, tab = ctx.octree_components(26, rt.MATCH_MATERIAL)
        seed = V[tab["first"][len(tab) // 2], :3]
        sel = dict(seeds=[seed], connectivity=26, match=rt.MATCH_MATERIAL)
        saved = ctx.octree_extract_connected(**sel)
        assert len(saved) == tab["voxels"][len(tab) // 2] and np.array_equal(saved, cm.extract(V, scene.max_depth, **sel))
        ctx.octree_edit_connected(rt.REGION_CLEAR, **sel)
        assert len(ctx.octree_extract_connected(**sel)) == 0
        ctx.octree_edit_voxels(rt.REGION_SET, saved)
        assert np.array_equal(vbos[0].read(np.uint32), compacted)
    finally:
        ctx.close()


# ---- 5. errors leave every byte as it was --------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    nc = ctypes.c_uint32(0)
    nv, ncomp = ctypes.c_size_t(0), ctypes.c_size_t(0)
    ok = rt.Select(6, 0, 0, 2**32 - 1, 0, 0)
    ctx = rt.Context(0)
    try:
        for bound in ((), (0,), (7,)):
            for s in bound:
                v = rt.VertexBufferObject(ctx, cells if s == 0 else np.array([depth, 64, 128], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, v)
            assert L.tdt_octree_components(ctx.h, 6, 0, None, 0, ctypes.byref(nv), None, 0, ctypes.byref(ncomp)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_edit_connected(ctx.h, rt.REGION_CLEAR, ctypes.byref(ok), None, 0, None, 0, 0, ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract_connected(ctx.h, ctypes.byref(ok), None, 0, None, 0, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        vbos = rt.upload_scene(ctx, scene)
        counter = rt.VertexBufferObject(ctx, np.array([777], np.uint32))
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)

        def unchanged():
            return np.array_equal(vbos[0].read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 777

        bad_shape = rt.box((0, 0, 0), (1, 1, 1))
        bad_shape.shape = 7
        E = ctx.octree_edit_connected
        cases = [lambda: E(rt.REGION_CLEAR, connectivity=18), lambda: E(rt.REGION_CLEAR, connectivity=0),
                 lambda: E(rt.REGION_CLEAR, match=2), lambda: E(rt.REGION_CLEAR, match=-1), lambda: E(rt.REGION_CLEAR, invert=2),
                 lambda: E(rt.REGION_CLEAR, min_voxels=5, max_voxels=4), lambda: E(rt.REGION_SET), lambda: E(rt.REGION_FILL),
                 lambda: E(7), lambda: E(rt.REGION_PAINT, material=254), lambda: E(rt.REGION_PAINT, material=-1),
                 lambda: E(rt.REGION_CLEAR, regions=bad_shape), lambda: E(rt.REGION_CLEAR, regions=rt.sphere((1, 1, 1), -1)),
                 lambda: ctx.octree_extract_connected(connectivity=8), lambda: ctx.octree_extract_connected(min_voxels=2, max_voxels=1),
                 lambda: ctx.octree_components(connectivity=4), lambda: ctx.octree_components(match=3)]
        for f in cases:
            with pytest.raises(rt.TdtError) as e:
                f()
            assert e.value.code == rt.ERR_INVALID_VALUE and unchanged()
        for rc in (L.tdt_octree_edit_connected(ctx.h, rt.REGION_CLEAR, ctypes.byref(ok), None, 1, None, 0, 0, ctypes.byref(nc)),
                   L.tdt_octree_edit_connected(ctx.h, rt.REGION_CLEAR, ctypes.byref(ok), None, 0, None, 1, 0, ctypes.byref(nc)),
                   L.tdt_octree_edit_connected(ctx.h, rt.REGION_CLEAR, None, None, 0, None, 0, 0, ctypes.byref(nc)),
                   L.tdt_octree_extract_connected(ctx.h, ctypes.byref(ok), None, 2, None, 0, None, 0, ctypes.byref(nv))):
            assert rc == rt.ERR_INVALID_VALUE and unchanged()
        # capacities below the counts: the counts set, nothing written
        V = ctx.octree_extract()
        want_l, want_t = cm.components(V, depth, 6, rt.MATCH_ANY)
        labels = np.full(len(V), 0xABCDEF, np.uint32)
        comps = np.zeros(len(want_t), rt.COMPONENT_DTYPE)
        comps["first"] = 99
        for lcap, ccap in ((len(V) - 1, len(comps)), (len(V), len(comps) - 1)):
            rc = L.tdt_octree_components(ctx.h, 6, 0, labels.ctypes.data, lcap, ctypes.byref(nv), comps.ctypes.data, ccap, ctypes.byref(ncomp))
            assert rc == rt.ERR_INVALID_VALUE and (nv.value, ncomp.value) == (len(V), len(want_t))
            assert (labels == 0xABCDEF).all() and (comps["first"] == 99).all()
        assert L.tdt_octree_components(ctx.h, 6, 0, None, 0, ctypes.byref(nv), None, 0, ctypes.byref(ncomp)) == rt.OK
        assert (nv.value, ncomp.value) == (len(V), len(want_t))
        seed = V[:1, :3]
        out = np.zeros((1, 4), np.int32)
        need = len(cm.extract(V, depth, seeds=seed))
        assert need > 1
        rc = L.tdt_octree_extract_connected(ctx.h, ctypes.byref(ok), np.ascontiguousarray(seed, np.int32).ctypes.data, 1, None, 0,
                                            out.ctypes.data, 1, ctypes.byref(nv))
        assert rc == rt.ERR_INVALID_VALUE and nv.value == need and not out.any()
        # a LEAF value >= 254 cannot be rebuilt (the labelling takes extract's limit)
        bad = cells.copy()
        bad[2 * int(np.flatnonzero(cells[1::2] == 2)[0])] = 254
        vbos[0].sub_data(0, bad)
        with pytest.raises(rt.TdtError) as e:
            ctx.octree_edit_connected(rt.REGION_CLEAR, seeds=seed)
        assert e.value.code == rt.ERR_INVALID_VALUE and np.array_equal(vbos[0].read(np.uint32), bad)
        ctx.octree_components()
        # a result larger than the buffer (possible only with shared cells: PAINT and CLEAR of whole components never split a
        # merged block): a depth-2 tree whose root points twice at one cell; n_cells reports what it needs
        shared = np.zeros(32, np.uint32)
        shared[0:2] = (1, 1)
        shared[14:16] = (1, 1)
        shared[16:18] = (4, 2)
        vbo, counter2 = bind_cells(ctx, shared, 2)
        ints = rt.VertexBufferObject(ctx, np.array([2, 64, 4], np.int32))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
        V2 = ctx.octree_extract()
        assert V2.tolist() == [[0, 0, 0, 5], [2, 2, 2, 5]]
        need = len(built_cells(ctx, V2, 2)) // 16
        assert need == 3
        for op in (rt.REGION_PAINT, rt.REGION_CLEAR):
            with pytest.raises(rt.TdtError) as e:
                ctx.octree_edit_connected(op, seeds=[(1, 1, 1)], material=4)      # a click on air: the tree as it is
            assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
            assert np.array_equal(vbo.read(np.uint32), shared) and int(counter2.read(np.uint32)[0]) == 12345
    finally:
        ctx.close()


# ---- 6. ordering and multi-device ----------------------------------------------------------------------------------------
def test_edit_dispatched_just_before_is_included(oracle):
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 3000, np.uint32)])
    d = distinct_deltas(np.random.default_rng(22), 200, depth, scene.blobs[0])
    d[:, 3], d[:, 4] = 2.0, 4.0
    edited, _ = oracle_py.oracle_octree_update(oracle, scene, d, used, (len(d), 1, 1))
    r, upd, counter = edit_setup(scene, used, d)
    try:
        ctx2 = rt.Context(0)
        try:
            v7 = rt.VertexBufferObject(ctx2, scene.blobs[7])
            ctx2.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, v7)
            bind_cells(ctx2, scene.blobs[0], len(scene.blobs[0]) // 16)
            V0 = ctx2.octree_extract()
            bind_cells(ctx2, edited, len(edited) // 16)
            V = ctx2.octree_extract()
            seed = V[~np.isin(morton(V[:, :3]), morton(V0[:, :3]))][0, :3]   # a voxel only the queued edit places
            want_vox = cm.edit(V, depth, rt.REGION_PAINT, 9, seeds=[seed])
            want, n_want = expected_bytes(ctx2, want_vox, depth, scene.blobs[0].nbytes)
        finally:
            ctx2.close()
        upd.dispatch_compute(len(d), 1, 1)                 # no finish
        n = r.ctx.octree_edit_connected(rt.REGION_PAINT, seeds=[seed], material=9)
        assert n == n_want and np.array_equal(r.vbos[0].read(np.uint32), want)
        assert int(counter.read(np.uint32)[0]) == n
    finally:
        r.close()


def test_multi_device_edit_connected_renders_like_a_single_device(oracle):
    scene = host.Scene.config(3)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            V = r.ctx.octree_extract()
            labels, tab = r.ctx.octree_components()
            seed = V[tab["first"][1], :3]
            n = r.ctx.octree_edit_connected(rt.REGION_CLEAR, seeds=[seed])
            n += r.ctx.octree_edit_connected(rt.REGION_PAINT, seeds=[V[0, :3]], match=rt.MATCH_MATERIAL, material=12)
            outs.append((n, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), labels, tab))
        finally:
            r.close()
    (n1, c1, img1, v1, l1, t1), (n2, c2, img2, v2, l2, t2) = outs
    assert n1 == n2 and np.array_equal(c1, c2) and np.array_equal(v1, v2)
    assert np.array_equal(l1, l2) and t1.tobytes() == t2.tobytes()
    assert (img1.view(np.uint32) == img2.view(np.uint32)).all()
    assert (img1.view(np.uint32) == oracle.render(host.Scene({**scene.blobs, 0: c1}), cam, threads=4).view(np.uint32)).all()


# ---- 7. the demo scene: the component table only -------------------------------------------------------------------------
def test_demo_scene_component_table():
    L = rt.lib()
    scene = host.Scene.demo()
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        voxels = ctx.octree_census()["voxels"]
        n = 1 << scene.max_depth
        nv, nc = ctypes.c_size_t(0), ctypes.c_size_t(0)
        ctx.check(L.tdt_octree_components(ctx.h, 6, 0, None, 0, ctypes.byref(nv), None, 0, ctypes.byref(nc)))
        assert nv.value == voxels > 200_000_000 and nc.value > 0
        tab = np.zeros(nc.value, rt.COMPONENT_DTYPE)
        ctx.check(L.tdt_octree_components(ctx.h, 6, 0, None, 0, ctypes.byref(nv), tab.ctypes.data, len(tab), ctypes.byref(nc)))
        assert int(tab["voxels"].astype(np.int64).sum()) == voxels
        assert (np.diff(tab["first"].astype(np.int64)) > 0).all() and tab["first"][0] == 0
        assert (tab["lo"] >= 0).all() and (tab["hi"] < n).all() and (tab["lo"] <= tab["hi"]).all()
        del vbos
    finally:
        ctx.close()


# ---- 8. the demo ---------------------------------------------------------------------------------------------------------
def test_demo_flood_clear_equals_the_oracle(oracle, tmp_path):
    exe = build.build_demo()
    out = str(tmp_path / "frame.pfm")
    w, h = 128, 96
    scene = host.Scene.config(3)
    depth = scene.max_depth
    cam = host.camera_reference_pose(w, h, 2, 6)
    r = rt.Renderer(scene, cam)
    try:
        xy = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.int32)
        picks = r.pick(xy)
        V = r.ctx.octree_extract()
    finally:
        r.close()
    labels, tab = cm.components(V, depth, 6, rt.MATCH_ANY)
    keys = morton(V[:, :3]).astype(np.int64)
    floor = int(np.argmax(tab["voxels"]))
    order = np.argsort(np.abs(xy[:, 0] - w // 2) + np.abs(xy[:, 1] - h // 2), kind="stable")
    room = len(np.asarray(scene.blobs[0]).view(np.uint32)) // 16          # the demo uploads the scene's cells buffer as it is
    px = None
    for i in order:                                                       # the pixel nearest the centre on a piece above the floor
        if not (picks[i]["status"] == rt.RAY_HIT and picks[i]["fresh_record"]):
            continue
        try:
            seed = host.pick_grid_voxel(picks[i], scene, 0)
        except ValueError:
            continue
        j = int(np.searchsorted(keys, int(morton(seed)[0])))
        if j < len(V) and keys[j] == int(morton(seed)[0]) and labels[j] != floor:
            px = xy[i]
            break
    assert px is not None, "precondition: a pixel on a piece above the floor"
    want_vox = cm.edit(V, depth, rt.REGION_CLEAR, seeds=[seed])
    assert len(want_vox) < len(V)
    ctx = rt.Context(0)
    try:
        built = built_cells(ctx, want_vox, depth)
    finally:
        ctx.close()
    assert len(built) // 16 <= room
    want, n = padded(built, 64 * room), len(built) // 16
    p = subprocess.run([exe, "--config", "3", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "6", "--pick", f"{px[0]},{px[1]}",
                        "--flood", "clear", "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"flood applied cells {n}\b", p.stdout), p.stdout
    ref = oracle.render(host.Scene({**scene.blobs, 0: want}), cam, threads=8)
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF4"
        fw, fh = map(int, f.readline().split())
        f.readline()
        img = np.frombuffer(f.read(), "<f4").reshape(fh, fw, 4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


# ---- 9. the wrappers: one labelling, a table grown on demand, empty filters, the size window -------------------------------
def test_wrappers_table_growth_empty_filters_and_the_demo_count():
    scene = host.Scene.config(3)
    depth = scene.max_depth
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        want_l, want_t = cm.components(V, depth, 6, rt.MATCH_ANY)
        assert len(want_t) == 20
        for capacity in (1, 19, 20, 4096):                  # below the count: the table is grown and the tree labelled again
            labels, tab = ctx.octree_components(capacity=capacity)
            assert np.array_equal(labels, want_l) and tab.tobytes() == want_t.tobytes(), capacity
        # an empty seed or region list selects nothing (None is no filter); invert then selects everything
        for kw in (dict(seeds=[]), dict(regions=[])):
            assert len(ctx.octree_extract_connected(**kw)) == 0
            assert np.array_equal(ctx.octree_extract_connected(invert=True, **kw), V)
            ctx.octree_edit_connected(rt.REGION_CLEAR, **kw)
            assert np.array_equal(ctx.octree_extract(), V)
        assert np.array_equal(ctx.octree_extract_connected(), V)
        for lo, hi in ((-1, 8), (0, 2**32)):
            with pytest.raises(ValueError):
                ctx.octree_edit_connected(rt.REGION_CLEAR, min_voxels=lo, max_voxels=hi)
        assert np.array_equal(ctx.octree_extract(), V)
        del vbos
    finally:
        ctx.close()
    exe = build.build_demo()
    for args, want in (([], "components 20 largest 422581"), (["--connect", "26", "--match", "material"], "components 240 largest 73525")):
        p = subprocess.run([exe, "--config", "3", "--size", "32x32", "--spp", "1", "--bounce", "1", "--components"] + args,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert re.search(rf"^{want}$", p.stdout, re.M), p.stdout
