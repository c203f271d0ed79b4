"""Affine transforms of voxel selections on the GPU (tdt_octree_transform / tdt_octree_extract_transform) against the dense numpy
model (tests/xform_model.py), everywhere by exact equality: lists as arrays, trees as the bytes tdt_octree_edit_voxels of the
model's list leaves, which are the builder's tree of the model's result."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import xform_model as xm
from test_gpu_connect import bind_tree, block
from test_gpu_distance import random_tree
from test_gpu_region_edit import OPS, apply_op, bind_cells, built_cells, padded, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
BIG = 2 ** 31 - 1
EDGES = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 126, 127)


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def same(got, want, tag=""):
    assert got.shape == want.shape and np.array_equal(got, want), tag


def tree_of(depth):
    """test_gpu_distance's balls with salt and pepper, plus voxels in the corners and on the x = N - 1 face, so that a move by
    -N + 1 keeps something under every variant."""
    n = 1 << depth
    extra = np.array([[0, 0, 0, 3], [n - 1, n - 1, n - 1, 250], [n - 1, 4, 3, 77], [n - 1, 5, 2, 78]], np.int32)
    V = random_tree(depth)
    keep = ~np.isin(V[:, :3] @ [n * n, n, 1], extra[:, :3] @ [n * n, n, 1])
    return sort_vox(np.concatenate([V[keep], extra]))


def mask_of(depth):
    n = 1 << depth
    return [rt.box((n // 2, 0, 2), (n - 1, n - 2, n - 1)), rt.sphere((n // 2, n // 2, n // 3), n // 3)]


def transforms(depth):
    """(tag, kind, transform): the suite's transforms on a grid of side N, the rotations and 3/2 about off-centre pivots."""
    n = 1 << depth
    c = (n, n, n)
    out = [("identity", "identity", xm.identity()), ("move 1 -3 5", "translate", xm.translate((1, -3, 5))),
           ("move -N+1", "translate", xm.translate((-n + 1, 0, 0)))]
    out += [(f"turn {axis} x{k}", "turn", xm.quarter_turns(axis, k, c)) for axis in range(3) for k in (1, 2, 3)]
    out += [(f"mirror {axis}", "mirror", xm.mirror(axis, (n - 1 + axis, n + 1, n))) for axis in range(3)]
    out += [("x2", "scale", xm.scale((2, 2, 2), (1, 1, 1), c)), ("x1/2", "scale", xm.scale((1, 1, 1), (2, 2, 2), (n // 2,) * 3)),
            ("x3/2", "scale", xm.scale((3, 3, 3), (2, 2, 2), (n - 3, n + 2, n)))]
    out += [("rotate 30", "rotate", xm.rotation((0, 0, 1), 30.0, (n / 2 + 0.5, n / 2 - 1.25, 0.0))),
            ("rotate 45", "rotate", xm.rotation((1, 1, 1), 45.0, (n / 2 - 0.75, n / 2 + 1.0, n / 2 + 0.5)))]
    return out


def variants(x, depth):
    """(tag, transform, regions, expected empty): no mask, a box + sphere mask, an empty mask, a material override, a destination
    box that cuts through bricks."""
    return [("plain", x, None, False), ("mask", x, mask_of(depth), False), ("empty mask", x, [], True),
            ("material", x.with_(material=17), None, False), ("dst", x.with_(dst_lo=[0, 3, 0], dst_hi=[BIG, 12, BIG]), None, False)]


def model_cases(depth):
    """Every (tag, transform, regions, model list) of a depth, each checked by the model alone to be worth running: non-empty
    (but under the empty mask) and not V itself (but the plain identity)."""
    V = tree_of(depth)
    cases = []
    for tag, _, x in transforms(depth):
        for vtag, xv, regions, empty in variants(x, depth):
            want = xm.transform(V, depth, xv, regions)
            assert (len(want) == 0) == empty, (depth, tag, vtag)
            assert empty or (tag, vtag) == ("identity", "plain") or not np.array_equal(want, V), (depth, tag, vtag)
            cases.append((f"{tag} / {vtag}", xv, regions, want))
    return V, cases


# ---- 1. random trees -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 4, 5, 6])
def test_random_trees_equal_the_model(ctx, depth):
    """Depth 3 is one brick, 4 is 2^3 bricks, 5 a partial word of the bit volume, 6 a word boundary at x = 31 / 32."""
    V, cases = model_cases(depth)
    vbo, counter, _ = bind_tree(ctx, V, depth)
    before = vbo.read(np.uint32)
    for tag, x, regions, want in cases:
        same(ctx.octree_extract_transform(x.fields(), regions), want, tag)
        kept, domain = ctx.xform_bricks()[::-1]
        assert kept <= domain <= 8 ** max(depth - 3, 0) and (kept > 0 or len(want) == 0), tag
    same(ctx.octree_extract(), V, "the tree is untouched")
    assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345


# ---- 2. the edit form ----------------------------------------------------------------------------------------------------------
def check_edit(ctx, V, depth, x, op, regions, tag):
    """octree_transform on a fresh tree of V: the bytes octree_edit_voxels(op, the model's list) leaves, which are the builder's
    tree of the model's result; the counter is the returned count."""
    T = xm.transform(V, depth, x, regions)
    want = apply_op(V, op, T, None)
    built = built_cells(ctx, want, depth, model=len(want) <= 1 << 16)
    have = len(built_cells(ctx, V, depth, model=False)) // 16
    room = max(len(built) // 16 - have, 0) + 8
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    n = ctx.octree_transform(x.fields(), op, regions)
    got = vbo.read(np.uint32)
    assert n == len(built) // 16 and int(counter.read(np.uint32)[0]) == n, tag
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    assert ctx.octree_edit_voxels(op, T) == n, tag
    assert np.array_equal(got, vbo.read(np.uint32)) and np.array_equal(got, padded(built, got.nbytes)), tag
    return want


@pytest.mark.parametrize("kind", ["translate", "turn", "mirror", "scale", "rotate"])
def test_edit_form_of_every_kind_and_op(ctx, kind):
    depth = 5
    V = tree_of(depth)
    picked = [(tag, x) for tag, k, x in transforms(depth) if k == kind]
    changed = set()
    for i, op in enumerate(OPS):
        tag, x = picked[i % len(picked)]
        regions = mask_of(depth) if i % 2 else None
        x = x.with_(material=9) if op == rt.REGION_PAINT else x
        want = check_edit(ctx, V, depth, x, op, regions, (tag, op))
        if not np.array_equal(want, V):
            changed.add(op)
    assert changed == set(OPS)                                  # by the model alone: every op did something


# ---- 3. brick and word boundaries, floor at -1 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_brick_and_word_boundaries(ctx, axis):
    depth, n = 7, 128
    V = np.zeros((len(EDGES), 4), np.int32)
    V[:, :3] = np.array([40, 77, 9])[None, :]
    V[:, axis] = EDGES
    V[:, 3] = 1 + np.arange(len(EDGES))
    V = sort_vox(V)
    bind_tree(ctx, V, depth)
    step = [0, 0, 0]
    for d in (1, -1):
        step[axis] = d
        want = xm.transform(V, depth, xm.translate(step))
        assert len(want) == len(V) - 1                          # the voxel at the face leaves the grid; nothing appears at the other
        same(ctx.octree_extract_transform(xm.translate(step).fields()), want, (axis, d))
    for turn_axis in range(3):
        x = xm.quarter_turns(turn_axis, 1, (n, n, n))
        want = xm.transform(V, depth, x)
        assert len(want) == len(V) and not np.array_equal(want, V)
        same(ctx.octree_extract_transform(x.fields()), want, (axis, "turn", turn_axis))
    same(ctx.octree_extract(), V, "the tree is untouched")


# ---- 4. depth 10 -----------------------------------------------------------------------------------------------------------------
def test_depth_10_shrink_large_entries_and_a_culled_domain(ctx):
    """Shrinking by 16 point-samples the grid; entries of +-2^20 make a q alone leave int32 (the sum is int64); with t near 2^40
    the true source voxels lie 255 * 2^15 voxels outside the grid while a sum wrapped to 32 bits would land on the tree's voxels;
    and one moved voxel has a domain of a few bricks."""
    depth, n = 10, 1024
    few = np.array([[0, 0, 0, 1], [1023, 1023, 1023, 2], [15, 31, 1023, 3], [16, 32, 1008, 4], [511, 15, 47, 5], [512, 512, 512, 6],
                    [1023, 0, 15, 7], [0, 1023, 1023, 8], [799, 815, 831, 9], [800, 816, 832, 10], [31, 1023, 527, 11], [1007, 15, 15, 12]], np.int32)
    V = sort_vox(few)
    bind_tree(ctx, V, depth)
    # shrink by 16: s = 16 p + 8 + t / 2^17, point sampling one voxel of every 16^3
    total = 0
    for off in (7, -8):
        x = xm.X([16 * 65536, 0, 0, 0, 16 * 65536, 0, 0, 0, 16 * 65536], [off * (1 << 17)] * 3, dst_lo=[0, 0, 0], dst_hi=[63, 63, 63])
        want = xm.transform(V, depth, x)
        total += len(want)
        assert len(want) >= 3
        same(ctx.octree_extract_transform(x.fields()), want, ("shrink", off))
        full = ctx.octree_extract_transform(x.with_(dst_hi=[BIG] * 3).fields())    # nothing of the grid beyond 63 has its source in it
        same(full, want, ("shrink, whole grid", off))
    assert total == 10                                           # by hand: the voxels with every coordinate = 15, or = 0, mod 16
    # entries of +-2^20: the 32-bit sum wraps
    A = 1 << 20
    x = xm.X([A, -A, 0, 0, A, -A, A, 0, A], [600 << 17, 500 << 17, -16300 << 17], dst_lo=[500, 500, 500], dst_hi=[531, 531, 531])
    p = np.stack(np.meshgrid(*[np.arange(500, 532)] * 3, indexing="ij"), -1).reshape(-1, 3)
    aq = (2 * p + 1) @ np.array(x.a, np.int64).reshape(3, 3).T
    assert (np.abs(aq) >= 2 ** 31).any()
    s = xm.source_of(x, p)
    landed = np.unique(s[((s >= 0) & (s < n)).all(1)], axis=0)
    assert len(landed) >= 100
    pick = landed[:: len(landed) // 40]
    W = sort_vox(np.concatenate([np.concatenate([pick, 1 + np.arange(len(pick))[:, None] % 254], 1), few[:2]]))
    bind_tree(ctx, W, depth)
    want = xm.transform(W, depth, x)
    assert len(want) >= len(pick) and len(set(want[:, 3])) > 20
    same(ctx.octree_extract_transform(x.fields()), want, "2^20 entries")
    far = x.with_(t=[v + 255 * 2 ** 32 for v in x.t])          # 2^40 - 2^32 and a bit: within the limit
    assert all(2 ** 39 < v <= 2 ** 40 for v in far.t)
    total = aq + np.array(far.t)
    wrapped = total.astype(np.int32).astype(np.int64)
    assert (wrapped != total).all() and np.array_equal(wrapped >> 17, s)      # a 32-bit sum would find every voxel again
    assert len(xm.transform(W, depth, far)) == 0
    for f in (far, far.with_(dst_lo=[0, 0, 0], dst_hi=[BIG] * 3)):
        assert len(ctx.octree_extract_transform(f.fields())) == 0
    # one voxel moved by (500, -20, 3): the domain comes from the preimage of the source box, not from the grid
    one = np.array([[100, 200, 300, 7]], np.int32)
    bind_tree(ctx, one, depth)
    x = xm.translate((500, -20, 3))
    want = xm.transform(one, depth, x.with_(dst_lo=[590, 170, 290], dst_hi=[610, 190, 310]))
    assert want.tolist() == [[600, 180, 303, 7]]
    same(ctx.octree_extract_transform(x.fields()), want, "one voxel")
    domain, kept = ctx.xform_bricks()
    assert 1 <= kept <= domain <= 27


# ---- 5. errors and limits ------------------------------------------------------------------------------------------------------
def test_empty_tree(ctx):
    depth = 4
    vbo, counter, _ = bind_tree(ctx, np.zeros((0, 4), np.int32), depth, 4)
    for _, _, x in transforms(depth)[:6]:
        assert len(ctx.octree_extract_transform(x.fields())) == 0
        assert ctx.xform_bricks() == (0, 0)
        for op in OPS:
            assert ctx.octree_transform(x.fields(), op) == 1
            assert not vbo.read(np.uint32).any() and int(counter.read(np.uint32)[0]) == 1


def test_errors_write_nothing(ctx):
    L = rt.lib()
    depth = 5
    V = tree_of(depth)
    nc, nv = ctypes.c_uint32(0), ctypes.c_size_t(0)
    ok = host.xform_translate((1, 0, 0))
    fresh = rt.Context(0)
    try:
        for bound in ((), (0,), (7,)):
            for s in bound:
                v = rt.VertexBufferObject(fresh, np.zeros(16, np.uint32) if s == 0 else np.array([depth, 64, 32], np.int32))
                fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, v)
            assert L.tdt_octree_transform(fresh.h, ctypes.byref(ok), rt.REGION_SET, None, 0, ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract_transform(fresh.h, ctypes.byref(ok), None, 0, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
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
    one = 65536
    M, E = ctx.octree_transform, ctx.octree_extract_transform
    bad = [dict(a=[0] * 9), dict(a=[one, 0, 0, one, 0, 0, 0, 0, one]), dict(a=[one, 2 * one, 3 * one, 4 * one, 5 * one, 6 * one, 7 * one, 8 * one, 9 * one]),
           dict(a=[(1 << 20) + 1, 0, 0, 0, one, 0, 0, 0, one]), dict(a=[one, 0, 0, 0, one, -(1 << 20) - 1, 0, 0, one]),
           dict(t=[(1 << 40) + 1, 0, 0]), dict(t=[0, 0, -(1 << 40) - 1]), dict(material=254), dict(material=-2), dict(pad=[0, 1]), dict(pad=[-1, 0])]
    cases = [lambda b=b: M(b) for b in bad] + [lambda b=b: E(b) for b in bad]
    cases += [lambda: M({}, op=4), lambda: M({}, op=-1), lambda: M({}, regions=bad_shape), lambda: E({}, regions=bad_shape),
              lambda: M({}, regions=rt.sphere((1, 1, 1), -1))]
    for i, f in enumerate(cases):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE and unchanged(), i
    for rc in (L.tdt_octree_transform(ctx.h, None, rt.REGION_SET, None, 0, ctypes.byref(nc)),
               L.tdt_octree_transform(ctx.h, ctypes.byref(ok), rt.REGION_SET, None, 1, ctypes.byref(nc)),
               L.tdt_octree_extract_transform(ctx.h, None, None, 0, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_transform(ctx.h, ctypes.byref(ok), None, 2, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_transform(ctx.h, ctypes.byref(ok), None, 0, None, 0, None),
               L.tdt_debug_xform_bricks(ctx.h, None)):
        assert rc == rt.ERR_INVALID_VALUE and unchanged()
    # the limits themselves are valid
    for good in (dict(a=[1 << 20, 0, 0, 0, -(1 << 20), 0, 0, 0, one]), dict(t=[1 << 40, -(1 << 40), 0]), dict(material=253)):
        E(good)
    # the extract form's short capacity: the count, nothing written
    want = xm.transform(V, depth, xm.translate((1, 0, 0)))
    out = np.zeros((len(want), 4), np.int32)
    assert L.tdt_octree_extract_transform(ctx.h, ctypes.byref(ok), None, 0, out.ctypes.data, len(want) - 1, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
    assert nv.value == len(want) > 1 and not out.any() and unchanged()
    # a LEAF value >= 254 cannot be rebuilt: both forms refuse it
    broken = cells.copy()
    leaf = np.flatnonzero((broken[1::2] == 2) & (broken[0::2] < 254))[0]
    broken[2 * int(leaf)] = 254
    vbo2, counter2 = bind_cells(ctx, broken, len(broken) // 16)
    for f in (lambda: M({}), lambda: E({})):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE
        assert np.array_equal(vbo2.read(np.uint32), broken) and int(counter2.read(np.uint32)[0]) == 12345
    # a FILL that does not fit: the cell count it needs, nothing written; the same call on a buffer of that size succeeds
    vbo3, counter3, V1 = bind_tree(ctx, np.array([[32, 32, 32, 5]], np.int32), 6)
    chain = vbo3.read(np.uint32)
    move = xm.translate((-1, 0, 0))                              # into the other half of the grid: a second chain of cells
    built = built_cells(ctx, apply_op(V1, rt.REGION_FILL, xm.transform(V1, 6, move), None), 6)
    need = len(built) // 16
    assert need > len(chain) // 16
    with pytest.raises(rt.TdtError) as e:
        M(move.fields(), rt.REGION_FILL)
    assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
    assert np.array_equal(vbo3.read(np.uint32), chain) and int(counter3.read(np.uint32)[0]) == 12345
    vbo3, counter3 = bind_cells(ctx, chain, need)
    assert M(move.fields(), rt.REGION_FILL) == need
    assert np.array_equal(vbo3.read(np.uint32), built) and int(counter3.read(np.uint32)[0]) == need


def test_result_cap(ctx):
    """A full 64^3 block at depth 10 enlarged 16 times would be 2^30 voxels: refused after the count pass, before the list is
    allocated; enlarged 4 times it is 2^24 and runs."""
    depth = 10
    V = sort_vox(block((0, 0, 0), (63, 63, 63), 5))
    built = built_cells(ctx, V, depth, model=False)
    vbo, counter = bind_cells(ctx, built, len(built) // 16 + 8)
    ints = rt.VertexBufferObject(ctx, np.array([depth, 64, 1 << depth], np.int32))
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
    cells = vbo.read(np.uint32)
    x16, x4 = xm.scale((16,) * 3, (1,) * 3, (0, 0, 0)), xm.scale((4,) * 3, (1,) * 3, (0, 0, 0))
    assert x16.a[0] == 4096 and x16.t == [0, 0, 0]
    for f in (lambda: ctx.octree_extract_transform(x16.fields()), lambda: ctx.octree_transform(x16.fields(), rt.REGION_SET)):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE and "2^26" in str(e.value)
        assert np.array_equal(vbo.read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 12345
    assert ctx.xform_bricks() == (1 << 21, 1 << 21)
    nv = ctypes.c_size_t(0)
    x = rt.Context._xform(x4.fields())
    assert rt.lib().tdt_octree_extract_transform(ctx.h, ctypes.byref(x), None, 0, None, 0, ctypes.byref(nv)) == 0 and nv.value == 1 << 24
    domain, kept = ctx.xform_bricks()                            # the domain is the preimage's box widened by a voxel
    assert kept == 1 << 15 and kept <= domain <= 33 ** 3


# ---- 6. a multi-device context ---------------------------------------------------------------------------------------------------
def test_two_share_multi_device_edit_reaches_both_replicas():
    """A two-share context shards the frame over its members, so the frame after the edit shows every replica's cells: it must be,
    bit for bit, the single-device frame after the same edit, and the cells those of a single context."""
    scene = host.Scene.config(2)
    depth = scene.max_depth
    n = 1 << depth
    full = sum(8 ** l for l in range(depth))                    # no tree of this depth has more cells: any result fits
    scene.blobs[0] = padded(np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), 64 * full)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    turn, move = xm.quarter_turns(1, 1, (n, n, n)), xm.translate((3, -2, 1)).with_(material=4)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            V = r.ctx.octree_extract()
            mask = [rt.sphere(V[len(V) // 2, :3].astype(int), 12)]
            preview = r.ctx.octree_extract_transform(turn.fields())
            n1 = r.ctx.octree_transform(turn.fields(), rt.REGION_SET)
            n2 = r.ctx.octree_transform(move.fields(), rt.REGION_FILL, mask)
            outs.append((n1, n2, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), preview))
            if devices:
                assert rt.lib().tdt_ctx_device_count(r.ctx.h) == 2
        finally:
            r.close()
    one, two = outs
    for k, (a, b) in enumerate(zip(one, two)):                  # counts, cells, frame (by its bits), tree, preview
        if isinstance(a, np.ndarray) and a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), k
    T = xm.transform(V, depth, turn)
    same(two[5], T, "preview")
    turned = apply_op(V, rt.REGION_SET, T, None)
    want = apply_op(turned, rt.REGION_FILL, xm.transform(turned, depth, move, mask), None)
    assert not np.array_equal(turned, V) and not np.array_equal(want, turned)
    same(two[4], want, "the tree after both edits")
    ctx = rt.Context(0)
    try:
        built = built_cells(ctx, want, depth, model=False)
    finally:
        ctx.close()
    assert two[1] == len(built) // 16 and np.array_equal(two[2], padded(built, 64 * full))


# ---- 7. the demo ---------------------------------------------------------------------------------------------------------------
def test_demo_transform_leaves_the_model_tree(tmp_path):
    exe = build.build_demo()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    n = 1 << depth
    room = len(np.asarray(scene.blobs[0]).view(np.uint32)) // 16
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        want = apply_op(V, rt.REGION_FILL, xm.transform(V, depth, xm.quarter_turns(2, 1, (n, n, n)).with_(material=9)), None)
        cells = len(built_cells(ctx, want, depth)) // 16
        del vbos
    finally:
        ctx.close()
    assert len(want) > len(V)
    p = subprocess.run([exe, "--config", "2", "--size", "64x48", "--spp", "1", "--bounce", "2", "--cells", str(max(room, cells)), "--transform",
                        "turn:2,1", "--op", "fill", "--material", "9", "--out", str(tmp_path / "frame.pfm")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"transform turn cells {cells}\b", p.stdout), p.stdout
