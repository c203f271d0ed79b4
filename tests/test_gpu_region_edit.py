"""Region edits (tdt_octree_edit_region / tdt_octree_edit_voxels / tdt_octree_extract_region): an edit must leave in the bound
cells buffer exactly the builder's tree of op(V, B) followed by zeros, where V is what tdt_octree_extract returns and B the
brush's voxel set — on built trees with merged LEAFs above the last level (where the reference's edit program follows a
material index as if it were a cell), on shared-cell trees and on edit sessions with dead cells alike."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_py
import tree_model
from octree_util import distinct_deltas, edit_setup, written_node
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPS = (rt.REGION_SET, rt.REGION_FILL, rt.REGION_PAINT, rt.REGION_CLEAR)


# ---- the numpy model -------------------------------------------------------------------------------------------------
def spread3(v):
    v = np.asarray(v, np.uint64)
    k = np.zeros_like(v)
    for b in range(10):
        k |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return k


def morton(xyz):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return (spread3(xyz[:, 0]) << np.uint64(2)) | (spread3(xyz[:, 1]) << np.uint64(1)) | spread3(xyz[:, 2])


def inside(xyz, regions):
    """The shape predicate in exact integers (python ints past int64's reach are not needed: |d| <= r is tested first)."""
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    m = np.zeros(len(p), bool)
    for g in regions:
        a, b = np.array(list(g.a), np.int64), np.array(list(g.b), np.int64)
        if g.shape == rt.SHAPE_BOX:
            m |= ((p >= a) & (p <= b)).all(1)
        else:
            r = int(b[0])
            d = p - a
            near = (np.abs(d) <= r).all(1)
            m |= near & ((d.astype(object) ** 2).sum(1) <= r * r if r > (1 << 20) else (d * d).sum(1) <= r * r)
    return m


def brush_voxels(regions, depth):
    """B: the shapes' voxels inside the grid, unique, as (n, 3) int64."""
    n = 1 << depth
    out = []
    for g in regions:
        if g.shape == rt.SHAPE_BOX:
            lo, hi = np.array(list(g.a), np.int64), np.array(list(g.b), np.int64)
        else:
            lo = np.array(list(g.a), np.int64) - g.b[0]
            hi = np.array(list(g.a), np.int64) + g.b[0]
        lo, hi = np.maximum(lo, 0), np.minimum(hi, n - 1)
        if (lo > hi).any():
            continue
        grid = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
        out.append(grid[inside(grid, [g])])
    if not out:
        return np.zeros((0, 3), np.int64)
    return np.unique(np.concatenate(out), axis=0)


def sort_vox(v):
    v = np.asarray(v, np.int32).reshape(-1, 4)
    return np.ascontiguousarray(v[np.argsort(morton(v[:, :3]), kind="stable")])


def apply_op(V, op, B, bm):
    """op(V, B) over voxel lists {x, y, z, m}: V from extract, B (n, 4) with its materials; the result Morton-sorted."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    B = np.asarray(B, np.int32).reshape(-1, 4)
    kv, kb = morton(V[:, :3]), morton(B[:, :3])
    in_b = np.isin(kv, kb)
    in_v = np.isin(kb, kv)
    if op == rt.REGION_SET:
        out = np.concatenate([V[~in_b], B])
    elif op == rt.REGION_FILL:
        out = np.concatenate([V, B[~in_v]])
    elif op == rt.REGION_PAINT:
        out = V.copy()
        order = np.argsort(kb)
        pos = np.searchsorted(kb[order], kv[in_b])
        out[in_b, 3] = B[order[pos], 3]
    else:
        out = V[~in_b]
    return sort_vox(out)


def expected_region(V, op, regions, material, depth):
    b = brush_voxels(regions, depth)
    B = np.concatenate([b, np.full((len(b), 1), material + 1, np.int64)], 1)
    return apply_op(V, op, B, material + 1)


MODEL_LIMIT = 1 << 20                         # voxels up to which an expected tree is also checked against the numpy builder


def built_cells(ctx, vox, depth, model=True):
    """The builder's tree of vox (one all-EMPTY root for no voxels) as uint32 words.  Lists of at most MODEL_LIMIT voxels must
    also come out as the bytes of the numpy builder (tests/tree_model.py), so that what the edit suites expect does not rest
    on the GPU builder alone (tests/test_gpu_tree_roots.py pins the two to each other on aimed cases; this does it on every
    list the suites really use).  model=False: for a list the model does not take (a position listed twice)."""
    if len(vox) == 0:
        return np.zeros(16, np.uint32)
    vbo, n = rt.octree_build_cells(ctx, np.ascontiguousarray(vox, np.int32), depth)
    built = vbo.read(np.uint32)
    if model and len(vox) <= MODEL_LIMIT:
        want = tree_model.build_cells(vox, depth)
        assert n == len(want) // 16 and built.size == want.size and np.array_equal(built, want), "the GPU builder differs from tree_model"
    return built


def padded(built, nbytes):
    out = np.zeros(nbytes // 4, np.uint32)
    out[: len(built)] = built
    return out


def expected_bytes(ctx, vox, depth, nbytes):
    """The builder's tree of vox followed by zeros up to nbytes, and its cell count."""
    built = built_cells(ctx, vox, depth)
    return padded(built, nbytes), len(built) // 16


def monument_scene():
    z = np.load(os.path.join(GOLDEN, "monu1_ply_320x240_spp2_b6.npz"))
    return host.Scene({s: z[f"blob_{s}"] for s in (0, 1, 2, 3, 4, 6, 7)})


def edit_session_scene():
    """config 2 after places and removes through the edit program: dead cells, and the counter past the tree."""
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 2000, np.uint32)])
    d = distinct_deltas(np.random.default_rng(3), 200, depth, scene.blobs[0])
    place = d.copy()
    place[:, 3], place[:, 4] = 2.0, 5.0
    remove = d[::2].copy()
    remove[:, 3], remove[:, 4] = 0.0, 0.0
    r, upd, counter = edit_setup(scene, used, np.zeros(8 * 200, np.float32))
    try:
        dv = rt.VertexBufferObject(r.ctx, np.zeros(8 * 200, np.float32))
        r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, dv)
        for batch in (place, remove):
            dv.sub_data(0, np.ascontiguousarray(batch, np.float32))
            upd.dispatch_compute(len(batch), 1, 1)
        scene.blobs[0] = r.vbos[0].read(np.uint32)
        c = int(counter.read(np.uint32)[0])
    finally:
        r.close()
    assert c > used
    return scene


def scene_by_name(name):
    if name == "demo":
        return host.Scene.demo()
    if name == "monument":
        return monument_scene()
    if name == "session":
        return edit_session_scene()
    return host.Scene.config(int(name[-1]))


def bind_cells(ctx, cells, n_cells):
    """A cells buffer of n_cells cells holding `cells`, bound to slot 0; and a counter bound at 12345."""
    buf = np.zeros(16 * n_cells, np.uint32)
    c = np.asarray(cells).view(np.uint32)[: len(buf)]
    buf[: len(c)] = c
    vbo = rt.VertexBufferObject(ctx, buf)
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, vbo)
    counter = rt.VertexBufferObject(ctx, np.array([12345], np.uint32))
    ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)
    return vbo, counter


def shape_cases(V, depth):
    """The five brushes of the contract, placed around an occupied voxel."""
    n = 1 << depth
    c = V[len(V) // 2, :3].astype(int) if len(V) else np.array([n // 2] * 3)
    return {
        "box_inside": [rt.box(np.maximum(c - 2, 0), np.minimum(c + 2, n - 1))],
        "box_edge": [rt.box((n - 3, c[1] - 2, -4), (n + 5, c[1] + 2, c[2] + 3))],
        "sphere_outside": [rt.sphere((c[0], c[1], -3), 6)],
        "empty_box": [rt.box((c[0] + 1, 0, 0), (c[0], n - 1, n - 1))],
        "two_shapes": [rt.sphere(c, 3), rt.box(c - (1, 4, 0), c + (2, 1, 3))],
    }


# ---- 1. every op and shape on several scenes ---------------------------------------------------------------------------
# (the demo scene is left out here: its shared cells expand to 235 M voxels, minutes of numpy per case)
@pytest.mark.parametrize("name", ["config1", "config2", "config3", "monument", "session"])
def test_region_edit_equals_the_numpy_model(name):
    scene = scene_by_name(name)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        for op in OPS:
            for case, regions in shape_cases(V, depth).items():
                want_vox = expected_region(V, op, regions, 7, depth)
                built = built_cells(ctx, want_vox, depth)
                n_want = len(built) // 16
                room = max(len(cells) // 16, n_want) + 8
                vbo, counter = bind_cells(ctx, cells, room)
                want = padded(built, 64 * room)
                n = ctx.octree_edit_region(op, regions, 7)
                tag = f"{name} op {op} {case}"
                assert n == n_want, tag
                assert int(counter.read(np.uint32)[0]) == n, tag
                assert np.array_equal(vbo.read(np.uint32), want), tag
                assert np.array_equal(ctx.octree_extract(), want_vox), tag
        del vbos
    finally:
        ctx.close()


# ---- 2. an edit inside a merged LEAF -----------------------------------------------------------------------------------
def merged_leaf_voxel(cells, depth):
    """The middle voxel of the first LEAF found above level depth - 1 (a block of >= 4^3 voxels), or None."""
    cells = np.asarray(cells, np.uint32).reshape(-1, 8, 2)
    cell, base = np.zeros(1, np.int64), np.zeros((1, 3), np.int64)
    child = np.array([[c >> 2, (c >> 1) & 1, c & 1] for c in range(8)], np.int64)
    for level in range(1, depth - 1):
        nodes = cells[cell]
        pos = base[:, None, :] * 2 + child[None]
        t = nodes[..., 1]
        leaf = np.argwhere(t == 2)
        if len(leaf):
            size = 1 << (depth - level)
            i, c = leaf[0]
            return pos[i, c] * size + size // 2
        par = t == 1
        cell, base = nodes[..., 0][par].astype(np.int64), pos[par]
    return None


def test_carving_inside_a_merged_leaf(oracle):
    cam = host.camera_reference_pose(96, 64, 2, 3)
    for scene in (host.Scene.config(2), host.Scene.config(3), monument_scene()):
        depth = scene.max_depth
        p = merged_leaf_voxel(scene.blobs[0], depth)
        if p is not None:
            break
    assert p is not None, "precondition: a scene with a LEAF above the last level"
    assert written_node(np.asarray(scene.blobs[0]).view(np.uint32), (p + 0.5) / (1 << depth), depth) is None
    scene.blobs[0] = np.concatenate([np.asarray(scene.blobs[0]).view(np.uint32), np.zeros(16 * 64, np.uint32)])
    r = rt.Renderer(scene, cam)
    try:
        r.render()                                   # derived tables of the tree as it was
        V = r.ctx.octree_extract()
        want_vox = expected_region(V, rt.REGION_CLEAR, [rt.box(p, p)], 0, depth)
        assert len(want_vox) == len(V) - 1
        want, n_want = expected_bytes(r.ctx, want_vox, depth, scene.blobs[0].nbytes)
        n = r.ctx.octree_edit_region(rt.REGION_CLEAR, rt.box(p, p))
        got = r.vbos[0].read(np.uint32)
        assert n == n_want and np.array_equal(got, want)
        img = r.render()
        ref = oracle.render(host.Scene({**scene.blobs, 0: got}), cam, threads=4)
        assert (img.view(np.uint32) == ref.view(np.uint32)).all()
    finally:
        r.close()


# ---- 3. the voxel-list form ------------------------------------------------------------------------------------------
def test_voxel_list_rules_and_multi_shape_equals_sequential():
    scene = host.Scene.config(2)
    depth = scene.max_depth
    n = 1 << depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    ctx = rt.Context(0)
    try:
        rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        room = len(cells) // 16 + 4096
        rng = np.random.default_rng(7)
        pts = np.concatenate([V[rng.choice(len(V), 40, replace=False), :3], rng.integers(0, n, (40, 3))]).astype(np.int32)
        lst = np.concatenate([pts, rng.integers(1, 255, (len(pts), 1))], 1).astype(np.int32)
        dup = lst[:20].copy()
        dup[:, 3] = rng.integers(1, 255, 20)                         # duplicates later in the list: these must win
        off = np.array([[-1, 3, 3, 9], [n, 0, 0, 9], [2, n + 5, 1, 9], [0, 0, -7, 9]], np.int32)
        stamp = np.concatenate([lst, off, dup]).astype(np.int32)
        last = {}
        for v in stamp:
            if (v[:3] >= 0).all() and (v[:3] < n).all():
                last[tuple(v[:3])] = v[3]
        B = np.array([[*k, m] for k, m in last.items()], np.int32)
        for op in OPS:
            want_vox = apply_op(V, op, B, 0)
            vbo, counter = bind_cells(ctx, cells, room)
            want, n_want = expected_bytes(ctx, want_vox, depth, 64 * room)
            s = stamp.copy()
            if op == rt.REGION_CLEAR:
                s[:, 3] = 999                                        # ignored
            assert ctx.octree_edit_voxels(op, s) == n_want
            assert np.array_equal(vbo.read(np.uint32), want), op
            assert np.array_equal(ctx.octree_extract(), want_vox), op
        # several shapes in one SET call == the same shapes one call at a time
        c = V[len(V) // 3, :3].astype(int)
        shapes = [rt.sphere(c, 4), rt.box(c - 3, c + 2), rt.sphere(c + 5, 2)]
        vbo, _ = bind_cells(ctx, cells, room)
        ctx.octree_edit_region(rt.REGION_SET, shapes, 11)
        together = vbo.read(np.uint32)
        vbo, _ = bind_cells(ctx, cells, room)
        for g in shapes:
            ctx.octree_edit_region(rt.REGION_SET, g, 11)
        assert np.array_equal(vbo.read(np.uint32), together)
    finally:
        ctx.close()


# ---- 4. region extract and undo --------------------------------------------------------------------------------------
def test_extract_region_and_undo():
    scene = host.Scene.config(3)
    depth = scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 4096, np.uint32)])     # room for the carved tree
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        original = vbos[0].read(np.uint32)
        V = ctx.octree_extract()
        c = V[len(V) // 2, :3].astype(int)
        regions = [rt.box(c - 6, c + 5), rt.sphere(c + (9, 0, 0), 5)]
        saved = ctx.octree_extract_region(regions)
        assert np.array_equal(saved, V[inside(V[:, :3], regions)])
        assert len(saved) > 0
        ctx.octree_edit_region(rt.REGION_CLEAR, regions)
        assert len(ctx.octree_extract_region(regions)) == 0
        ctx.octree_edit_voxels(rt.REGION_SET, saved)
        assert np.array_equal(vbos[0].read(np.uint32), original)
        assert len(ctx.octree_extract_region([])) == 0
    finally:
        ctx.close()


# ---- 5. errors leave every byte as it was ----------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    nc = rt.ctypes.c_uint32(0)
    ctx = rt.Context(0)
    try:
        box = rt.box((1, 1, 1), (3, 3, 3))
        for bound in ((), (0,), (7,)):
            for s in bound:
                v = rt.VertexBufferObject(ctx, cells if s == 0 else np.array([depth, 64, 128], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, v)
            assert L.tdt_octree_edit_region(ctx.h, 0, rt.ctypes.byref(box), 1, 1, rt.ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_edit_voxels(ctx.h, 0, None, 0, rt.ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        vbos = rt.upload_scene(ctx, scene)
        counter = rt.VertexBufferObject(ctx, np.array([777], np.uint32))
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)
        n = 1 << depth

        def unchanged():
            return np.array_equal(vbos[0].read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 777

        whole = rt.box((0, 0, 0), (n - 1, n - 1, n - 1))
        bad_shape = rt.box((0, 0, 0), (1, 1, 1))
        bad_shape.shape = 7
        cases = [lambda: ctx.octree_edit_region(4, whole, 1), lambda: ctx.octree_edit_region(-1, whole, 1),
                 lambda: ctx.octree_edit_region(rt.REGION_SET, bad_shape, 1),
                 lambda: ctx.octree_edit_region(rt.REGION_SET, rt.sphere((1, 1, 1), -1), 1),
                 lambda: ctx.octree_edit_region(rt.REGION_SET, whole, 254), lambda: ctx.octree_edit_region(rt.REGION_SET, whole, -1),
                 lambda: ctx.octree_edit_voxels(rt.REGION_SET, [[1, 1, 1, 0]]), lambda: ctx.octree_edit_voxels(rt.REGION_SET, [[1, 1, 1, 255]]),
                 lambda: ctx.octree_edit_voxels(7, [[1, 1, 1, 1]])]
        for f in cases:
            with pytest.raises(rt.TdtError) as e:
                f()
            assert e.value.code == rt.ERR_INVALID_VALUE and unchanged()
        # the brush cap: SET / FILL shapes enumerating more than 2^26 candidates together (PAINT / CLEAR enumerate nothing)
        big = scene_by_name("config5")
        vb5 = rt.upload_scene(ctx, big)
        n5 = 1 << big.max_depth
        whole5 = rt.box((0, 0, 0), (n5 - 1, n5 - 1, n5 - 1))
        k = rt.REGION_BRUSH_CAP // n5 ** 3 + 1
        before = vb5[0].read(np.uint32)
        for op in (rt.REGION_SET, rt.REGION_FILL):
            with pytest.raises(rt.TdtError) as e:
                ctx.octree_edit_region(op, [whole5] * k, 1)
            assert e.value.code == rt.ERR_INVALID_VALUE
        assert np.array_equal(vb5[0].read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 777
        del vb5
        # a LEAF value >= 254 cannot be rebuilt
        vbos = rt.upload_scene(ctx, scene)
        bad = cells.copy()
        bad[2 * int(np.flatnonzero(cells[1::2] == 2)[0])] = 254
        vbos[0].sub_data(0, bad)
        with pytest.raises(rt.TdtError) as e:
            ctx.octree_edit_region(rt.REGION_CLEAR, box, 0)
        assert e.value.code == rt.ERR_INVALID_VALUE and np.array_equal(vbos[0].read(np.uint32), bad)
        # a result larger than the buffer (one all-EMPTY root cell): n_cells reports what it needs
        root = rt.VertexBufferObject(ctx, np.zeros(16, np.uint32))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, root)
        ints = rt.VertexBufferObject(ctx, np.array([4, 64, 1 << 10], np.int32))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
        ball = rt.sphere((8, 8, 8), 3)
        need = len(built_cells(ctx, expected_region(np.zeros((0, 4), np.int32), rt.REGION_SET, [ball], 3, 4), 4)) // 16
        assert need > 1
        with pytest.raises(rt.TdtError) as e:
            ctx.octree_edit_region(rt.REGION_SET, ball, 3)
        assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
        assert not root.read(np.uint32).any() and int(counter.read(np.uint32)[0]) == 777
    finally:
        ctx.close()


def test_two_member_failures_report_like_a_single_device():
    """On a two-member context: the slot text before any member is touched, and a misfit on the first member reporting the cell
    count it needs, nothing written on either replica."""
    ctx = rt.Context(0, devices=[0, 0])
    try:
        ball = rt.sphere((8, 8, 8), 3)
        with pytest.raises(rt.TdtError, match="no buffer bound to shader-storage slot 0") as e:
            ctx.octree_edit_region(rt.REGION_SET, ball, 3)
        assert e.value.code == rt.ERR_INCOMPLETE and e.value.n_cells == 0
        root, counter = bind_cells(ctx, np.zeros(16, np.uint32), 1)
        with pytest.raises(rt.TdtError, match="no buffer bound to shader-storage slot 7") as e:
            ctx.octree_edit_region(rt.REGION_SET, ball, 3)
        assert e.value.code == rt.ERR_INCOMPLETE and e.value.n_cells == 0
        ints = rt.VertexBufferObject(ctx, np.array([4, 64, 1 << 10], np.int32))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
        need = len(built_cells(ctx, expected_region(np.zeros((0, 4), np.int32), rt.REGION_SET, [ball], 3, 4), 4)) // 16
        assert need > 1
        with pytest.raises(rt.TdtError, match="does not fit") as e:
            ctx.octree_edit_region(rt.REGION_SET, ball, 3)
        assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
        assert not root.read(np.uint32).any() and int(counter.read(np.uint32)[0]) == 12345
    finally:
        ctx.close()


# ---- 6. ordering -----------------------------------------------------------------------------------------------------
def test_edit_dispatched_just_before_is_included(oracle):
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 3000, np.uint32)])
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
            c = V[len(V) // 2, :3].astype(int)
            regions = [rt.sphere(c, 5)]
            want_vox = expected_region(V, rt.REGION_SET, regions, 9, depth)
            want, n_want = expected_bytes(ctx2, want_vox, depth, scene.blobs[0].nbytes)
        finally:
            ctx2.close()
        upd.dispatch_compute(len(d), 1, 1)                 # no finish
        n = r.ctx.octree_edit_region(rt.REGION_SET, regions, 9)
        assert n == n_want and np.array_equal(r.vbos[0].read(np.uint32), want)
        assert int(counter.read(np.uint32)[0]) == n
    finally:
        r.close()


# ---- 7. multi-device -------------------------------------------------------------------------------------------------
def test_multi_device_region_edit_renders_like_a_single_device(oracle):
    scene = host.Scene.config(2)
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 2000, np.uint32)])
    cam = host.camera_reference_pose(96, 64, 2, 3)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            V = r.ctx.octree_extract()
            c = V[len(V) // 2, :3].astype(int)
            n = r.ctx.octree_edit_region(rt.REGION_CLEAR, [rt.sphere(c, 6)], 0)
            n += r.ctx.octree_edit_region(rt.REGION_SET, [rt.box(c - 2, c + 2)], 12)
            outs.append((n, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract()))
        finally:
            r.close()
    (n1, c1, img1, v1), (n2, c2, img2, v2) = outs
    assert n1 == n2 and np.array_equal(c1, c2) and np.array_equal(v1, v2)
    assert (img1.view(np.uint32) == img2.view(np.uint32)).all()
    assert (img1.view(np.uint32) == oracle.render(host.Scene({**scene.blobs, 0: c1}), cam, threads=4).view(np.uint32)).all()


# ---- 8. the demo -----------------------------------------------------------------------------------------------------
def test_demo_brush_clear_equals_the_oracle(oracle, tmp_path):
    exe = build.build_demo()
    out = str(tmp_path / "frame.pfm")
    w, h = 128, 96
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cam = host.camera_reference_pose(w, h, 2, 6)
    r = rt.Renderer(scene, cam)
    try:
        xy = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.int32)
        picks = r.pick(xy)
        V = r.ctx.octree_extract()
    finally:
        r.close()
    order = np.argsort(np.abs(xy[:, 0] - w // 2) + np.abs(xy[:, 1] - h // 2), kind="stable")
    room = len(np.asarray(scene.blobs[0]).view(np.uint32)) // 16          # the demo uploads the scene's cells buffer as it is
    px = None
    ctx = rt.Context(0)
    try:
        tried, seen = 0, set()
        for i in order:
            if not (picks[i]["status"] == rt.RAY_HIT and picks[i]["fresh_record"]):
                continue
            try:
                centre = host.pick_grid_voxel(picks[i], scene, 0)
            except ValueError:
                continue
            if tuple(centre) in seen:
                continue
            seen.add(tuple(centre))
            want_vox = expected_region(V, rt.REGION_CLEAR, [rt.sphere(centre, 3)], 0, depth)
            built = built_cells(ctx, want_vox, depth)
            tried += 1
            if len(want_vox) < len(V) and len(built) // 16 <= room:    # a carve that fits the demo's buffer
                px, want, n = xy[i], padded(built, 64 * room), len(built) // 16
                break
            if tried == 200:
                break
    finally:
        ctx.close()
    assert px is not None, "precondition: a pixel whose carve fits the demo's cells buffer"
    p = subprocess.run([exe, "--config", "2", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "6", "--pick", f"{px[0]},{px[1]}",
                        "--brush", "sphere:3", "--op", "clear", "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"brush applied cells {n}\b", p.stdout), p.stdout
    ref = oracle.render(host.Scene({**scene.blobs, 0: want}), cam, threads=8)
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF4"
        fw, fh = map(int, f.readline().split())
        f.readline()
        img = np.frombuffer(f.read(), "<f4").reshape(fh, fw, 4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()
