"""Through-selection on the GPU (tdt_octree_extract_screen / tdt_octree_edit_screen / tdt_debug_screen_counts), bit for bit against
the numpy model (tests/screen_select_model.py): the list's bytes and the four counts for every shape, with and without the window
rule and the filters, on trees whose voxel counts sit on the wave and block edges; the cells buffer after PAINT and CLEAR; the
errors, which write nothing; and a two-member context."""
import ctypes

import numpy as np
import pytest

import screen_select_cases as cases
import screen_select_model as model
from image_util import _wrapped
from test_gpu_connect import bind_tree
from test_gpu_region_edit import built_cells, padded
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu
F = np.float32
TREES = ("n1", "n63", "n64", "n65", "n255", "n256", "n257", "n2048", "d10")
CAMS = ("outside", "inside", "centre")


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def bind(ctx, tree, floats, room=0):
    """The builder's tree of a case bound to slots 0 and 7, its OctreeFloats to slot 6; returns (cells vbo, counter, depth, V, floats)."""
    depth, V = cases.trees()[tree]
    vbo, counter, V = bind_tree(ctx, V, depth, room)
    fl = rt.VertexBufferObject(ctx, cases.FLOATS[floats])
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 6, fl)
    ctx._keep6 = fl
    return vbo, counter, depth, V, cases.FLOATS[floats]


def c_view(view):
    return rt.VIEW((ctypes.c_float * 3)(*view["origin"]), (ctypes.c_float * 3)(*view["lower_left_corner"]), (ctypes.c_float * 3)(*view["horizontal"]),
                   (ctypes.c_float * 3)(*view["vertical"]), view["image_width"], view["image_height"])


def c_sel(sel):
    return rt.ScreenSelect(sel["shape"], (ctypes.c_int32 * 4)(*sel["rect"]), sel["flags"], sel["material"], float(sel["min_distance"]),
                           float(sel["max_distance"]))


def c_polygon(polygon):
    if polygon is None:
        return None, 0, None
    p = np.ascontiguousarray(polygon, np.int32).reshape(-1, 2)
    return p.ctypes.data, len(p), p


class Masks:
    """The mask images of a context, uploaded once per (size, seed, kind)."""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, {}

    def of(self, key, array):
        if array is None:
            return None
        if key not in self.held:
            self.held[key] = _wrapped(self.ctx, array)
        return self.held[key][1]


def extract(ctx, view, sel, polygon, mask, capacity):
    """The raw call: (rc, list, count)."""
    out = np.zeros((max(capacity, 1), 4), np.int32)
    n = ctypes.c_size_t(0)
    pp, pn, keep = c_polygon(polygon)
    rc = rt.lib().tdt_octree_extract_screen(ctx.h, ctypes.byref(c_view(view)), ctypes.byref(c_sel(sel)), pp, pn, mask.h if mask is not None else None,
                                            out.ctypes.data, capacity, ctypes.byref(n))
    del keep
    return rc, out[: n.value] if rc == 0 else out, n.value


def edit(ctx, op, view, sel, polygon, mask, material=0):
    nc = ctypes.c_uint32(0)
    pp, pn, keep = c_polygon(polygon)
    rc = rt.lib().tdt_octree_edit_screen(ctx.h, op, ctypes.byref(c_view(view)), ctypes.byref(c_sel(sel)), pp, pn, mask.h if mask is not None else None,
                                         material, ctypes.byref(nc))
    del keep
    return rc, nc.value


def check_extract(ctx, masks, V, depth, fl, view, W, H, name, spec, tag, **kw):
    sel_kw, polygon, mask = spec
    sel = model.sel_of(**sel_kw, **kw)
    want, counts = model.extract(V, fl, cases.ints_of(depth), view, sel, polygon, mask)
    rc, got, n = extract(ctx, view, sel, polygon, masks.of((W, H, name), mask), len(V))
    assert rc == 0, (tag, rt.lib().tdt_last_error(ctx.h))
    assert n == len(want) and got.tobytes() == want.tobytes(), (tag, n, len(want))
    assert ctx.screen_counts() == counts, (tag, ctx.screen_counts(), counts)
    return want, counts


# ---- 1. every shape, both rules, on every tree, image and camera --------------------------------------------------------------------
@pytest.mark.parametrize("tree", TREES)
def test_extract_is_the_model(ctx, tree):
    """Per tree, the nine (image, camera) pairs share the twelve shapes with and without the window rule between them: every pair runs
    eight of the twenty-four, a different eight each, so every (shape, rule) runs on three pairs."""
    masks = Masks(ctx)
    floats = "odd" if TREES.index(tree) % 2 else "unit"
    _, _, depth, V, fl = bind(ctx, tree, floats)
    combos = [(s, w) for w in (False, True) for s in cases.shapes(4, 4)]
    seen, pair = set(), 0
    for W, H in cases.IMAGES:
        views = cases.cameras(V, depth, fl, W, H)
        shapes = cases.shapes(W, H)
        for cam in CAMS:
            for j in range(8):
                name, window = combos[(pair * 8 + j) % len(combos)]
                check_extract(ctx, masks, V, depth, fl, views[cam], W, H, name, shapes[name], (tree, W, H, cam, name, window), window=window)
                seen.add((name, window))
            pair += 1
    assert len(seen) == 24


def test_rect_polygon_and_mask_of_one_rectangle_give_the_same_bytes_on_the_device(ctx):
    masks = Masks(ctx)
    _, _, depth, V, fl = bind(ctx, "n2048", "odd")
    for W, H in cases.IMAGES[1:]:
        shapes = cases.shapes(W, H)
        for cam in ("outside", "inside"):
            view = cases.cameras(V, depth, fl, W, H)[cam]
            for window in (False, True):
                got = []
                for name in ("rect-part", "poly-rect", "mask-rect"):
                    sel_kw, polygon, mask = shapes[name]
                    rc, lst, n = extract(ctx, view, model.sel_of(**sel_kw, window=window), polygon, masks.of((W, H, name), mask), len(V))
                    assert rc == 0
                    got.append((lst.tobytes(), ctx.screen_counts()))
                assert got[0] == got[1] == got[2], (W, H, cam, window)
                assert got[0][1][3] > 0 or window


# ---- 2. the filters -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree,floats", [("n256", "unit"), ("n257", "odd")])
def test_filters(ctx, tree, floats):
    """A material that matches nothing, something and (n256 is of one material) everything; distance ranges that cut the set."""
    masks = Masks(ctx)
    _, _, depth, V, fl = bind(ctx, tree, floats)
    W, H = 64, 48
    shapes = cases.shapes(W, H)
    view = cases.cameras(V, depth, fl, W, H)["outside"]
    absent = next(m for m in range(254) if m + 1 not in set(V[:, 3].tolist()))
    cut = float(fl[4]) * 1.4                                       # between the nearest and the farthest voxel of this camera
    for name in ("rect-all", "poly-circle", "mask-random"):
        for window in (False, True):
            base, bc = check_extract(ctx, masks, V, depth, fl, view, W, H, name, shapes[name], (tree, name, window, "base"), window=window)
            assert bc[3] > 0
            present = int(base[len(base) // 2, 3]) - 1            # a material of the unfiltered selection
            for kw in (dict(material=absent), dict(material=present), dict(max_distance=cut), dict(min_distance=cut),
                       dict(min_distance=cut * 0.9, max_distance=cut * 1.1, material=present)):
                got, gc = check_extract(ctx, masks, V, depth, fl, view, W, H, name, shapes[name], (tree, name, window, kw), window=window, **kw)
                assert gc[:3] == bc[:3]
                if kw == dict(material=absent):
                    assert gc[3] == 0
                if kw == dict(material=present):
                    assert 0 < gc[3] and (gc[3] == bc[3]) == (tree == "n256")
                if set(kw) in ({"max_distance"}, {"min_distance"}):
                    assert 0 < gc[3] < bc[3], (name, window, kw, gc, bc)


# ---- 3. edits -----------------------------------------------------------------------------------------------------------------------
def cells_state(vbo, counter):
    return vbo.read(np.uint32), int(counter.read(np.uint32)[0])


@pytest.mark.parametrize("tree,floats", [("n65", "unit"), ("n257", "odd"), ("n2048", "unit")])
def test_paint_and_clear_leave_the_models_canonical_tree(ctx, tree, floats):
    masks = Masks(ctx)
    W, H = 33, 17
    shapes = cases.shapes(W, H)
    depth, V0 = cases.trees()[tree]
    views = cases.cameras(V0, depth, cases.FLOATS[floats], W, H)
    in_circle, _ = model.extract(V0, cases.FLOATS[floats], cases.ints_of(depth), views["outside"], model.sel_of(model.POLYGON), shapes["poly-circle"][1])
    plan = [("rect-part", "outside", False, {}), ("poly-triangle", "inside", False, {}), ("mask-random", "outside", True, {}),
            ("poly-circle", "outside", False, dict(material=int(in_circle[len(in_circle) // 2, 3]) - 1)), ("rect-empty", "outside", False, {})]
    for name, cam, window, kw in plan:
        sel_kw, polygon, mask = shapes[name]
        sel = model.sel_of(**sel_kw, window=window, **kw)
        for op in (rt.REGION_PAINT, rt.REGION_CLEAR):
            vbo, counter, depth, V, fl = bind(ctx, tree, floats, room=8)
            want, counts = model.edit(V, fl, cases.ints_of(depth), views[cam], sel, polygon, mask, op, 200)
            built = built_cells(ctx, want, depth)
            before = vbo.read(np.uint32)
            rc, nc = edit(ctx, op, views[cam], sel, polygon, masks.of((W, H, name), mask), 200)
            assert rc == 0, (tree, name, op)
            cells, count = cells_state(vbo, counter)
            assert nc == count == len(built) // 16 and np.array_equal(cells, padded(built, cells.nbytes)), (tree, name, op)
            assert ctx.screen_counts() == counts
            if name == "rect-empty":
                assert counts[3] == 0 and np.array_equal(cells, before)          # (the bound tree is the builder's: already canonical)
            else:
                assert counts[3] > 0 and not np.array_equal(cells, before), (tree, name, op)


def test_extract_then_clear_voxels_is_edit_screen_clear(ctx):
    W, H = 64, 48
    _, polygon, _ = cases.shapes(W, H)["poly-circle"]
    sel = model.sel_of(model.POLYGON, window=True)
    results = []
    for way in ("list", "screen"):
        vbo, counter, depth, V, fl = bind(ctx, "n2048", "odd", room=8)
        view = cases.cameras(V, depth, fl, W, H)["outside"]
        if way == "list":
            lst = ctx.octree_extract_screen(c_view(view), polygon=np.array(polygon, np.int32), window=True)
            assert 0 < len(lst) < len(V)
            nc = ctx.octree_edit_voxels(rt.REGION_CLEAR, lst)
        else:
            nc = ctx.octree_edit_screen(rt.REGION_CLEAR, c_view(view), polygon=np.array(polygon, np.int32), window=True)
            assert ctx.screen_counts()[3] == len(lst)
        results.append((nc, *cells_state(vbo, counter)))
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1]) and results[0][2] == results[1][2]
    assert sel["flags"] == rt.SCREEN_WINDOW


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing_and_keep_the_counts(ctx):
    L = rt.lib()
    W, H = 33, 17
    masks = Masks(ctx)
    vbo, counter, depth, V, fl = bind(ctx, "n257", "unit", room=4)
    view = cases.cameras(V, depth, fl, W, H)["outside"]
    good = model.sel_of(model.RECT, rect=(0, 0, W - 1, H - 1))
    rc, lst, n = extract(ctx, view, good, None, None, len(V))
    assert rc == 0 and n > 0
    counts = ctx.screen_counts()
    cells, count = cells_state(vbo, counter)
    tri = [(0, 0), (W, 0), (0, H)]
    mask = masks.of("m", np.ones((H, W, 4), F))
    small = masks.of("small", np.ones((H, W - 1, 4), F))

    def unchanged():
        c, k = cells_state(vbo, counter)
        return np.array_equal(c, cells) and k == count == 12345 and ctx.screen_counts() == counts

    def both(code, view=view, sel=good, polygon=None, mask=None, tag=""):
        rc, out, _ = extract(ctx, view, sel, polygon, mask, len(V))
        assert rc == code and not out.any() and unchanged(), ("extract", tag, rc)
        rc, _ = edit(ctx, rt.REGION_CLEAR, view, sel, polygon, mask)
        assert rc == code and unchanged(), ("edit", tag, rc)

    def sel(**kw):
        s = dict(good)
        s.update(kw)
        return s

    INV = rt.ERR_INVALID_VALUE
    both(INV, sel=sel(shape=3), tag="shape 3")
    both(INV, sel=sel(shape=-1), tag="shape -1")
    both(INV, sel=sel(flags=2), tag="flags")
    both(INV, sel=sel(flags=0x80000001), tag="flags high")
    both(INV, sel=sel(material=254), tag="material 254")
    both(INV, sel=sel(material=-2), tag="material -2")
    for lo, hi in ((np.nan, 1.0), (0.0, np.nan), (-1.0, 1.0), (0.0, -1.0), (2.0, 1.0), (-0.5, np.inf)):
        both(INV, sel=sel(min_distance=F(lo), max_distance=F(hi)), tag=("distance", lo, hi))
    poly = sel(shape=model.POLYGON)
    both(INV, sel=poly, polygon=None, tag="null polygon")
    both(INV, sel=poly, polygon=tri[:2], tag="2 vertices")
    both(INV, sel=poly, polygon=[(i, i % 5) for i in range(257)], tag="257 vertices")
    both(INV, sel=poly, polygon=[(0, 0), (W, 0), (0, (1 << 20) + 1)], tag="coordinate")
    both(INV, sel=poly, polygon=[(0, 0), (-(1 << 20) - 1, 0), (0, H)], tag="coordinate -")
    both(INV, sel=sel(shape=model.MASK), mask=None, tag="null mask")
    both(INV, sel=sel(shape=model.MASK), mask=small, tag="mask size")
    for w, h in ((1, H), (W, 1), (0, 0), (-3, H), ((1 << 24) + 1, H)):
        v = dict(view)
        v["image_width"], v["image_height"] = w, h
        both(INV, view=v, tag=("image", w, h))
    flat = dict(view)
    flat["horizontal"] = np.zeros(3, F)
    both(INV, view=flat, tag="degenerate view")
    nanv = dict(view)
    nanv["origin"] = np.array([np.nan, 0, 0], F)
    both(INV, view=nanv, tag="nan view")
    # null pointers; the edit's own arguments
    cv, cs = c_view(view), c_sel(good)
    nv, nc = ctypes.c_size_t(0), ctypes.c_uint32(0)
    assert L.tdt_octree_extract_screen(None, ctypes.byref(cv), ctypes.byref(cs), None, 0, None, None, 0, ctypes.byref(nv)) == INV
    assert L.tdt_octree_extract_screen(ctx.h, None, ctypes.byref(cs), None, 0, None, None, 0, ctypes.byref(nv)) == INV and unchanged()
    assert L.tdt_octree_extract_screen(ctx.h, ctypes.byref(cv), None, None, 0, None, None, 0, ctypes.byref(nv)) == INV and unchanged()
    assert L.tdt_octree_extract_screen(ctx.h, ctypes.byref(cv), ctypes.byref(cs), None, 0, None, None, 0, None) == INV and unchanged()
    assert L.tdt_octree_edit_screen(None, rt.REGION_CLEAR, ctypes.byref(cv), ctypes.byref(cs), None, 0, None, 0, ctypes.byref(nc)) == INV
    assert L.tdt_octree_edit_screen(ctx.h, rt.REGION_CLEAR, None, ctypes.byref(cs), None, 0, None, 0, ctypes.byref(nc)) == INV and unchanged()
    assert L.tdt_octree_edit_screen(ctx.h, rt.REGION_CLEAR, ctypes.byref(cv), None, None, 0, None, 0, ctypes.byref(nc)) == INV and unchanged()
    assert L.tdt_debug_screen_counts(None, (ctypes.c_uint64 * 4)()) == INV and L.tdt_debug_screen_counts(ctx.h, None) == INV
    for op in (rt.REGION_SET, rt.REGION_FILL, -1, 4):
        assert edit(ctx, op, view, good, None, None)[0] == INV and unchanged(), op
    for m in (-1, 254):
        assert edit(ctx, rt.REGION_PAINT, view, good, None, None, m)[0] == INV and unchanged(), m
        assert edit(ctx, rt.REGION_CLEAR, view, good, None, None, m)[0] == INV and unchanged(), m
    # a short capacity: the count, nothing written
    out = np.zeros((n, 4), np.int32)
    assert L.tdt_octree_extract_screen(ctx.h, ctypes.byref(cv), ctypes.byref(cs), None, 0, None, out.ctypes.data, n - 1, ctypes.byref(nv)) == INV
    assert nv.value == n and not out.any() and unchanged()
    # a NULL array only counts, and is a call that succeeds
    assert L.tdt_octree_extract_screen(ctx.h, ctypes.byref(cv), ctypes.byref(cs), None, 0, None, None, 0, ctypes.byref(nv)) == 0 and nv.value == n
    # an unused polygon or mask is ignored: even a bad one
    rc, got, k = extract(ctx, view, good, tri[:2], small, len(V))
    assert rc == 0 and got.tobytes() == lst.tobytes() and unchanged()
    # a mask of another context
    other = rt.Context(0)
    try:
        foreign = rt.Texture.new_2d(other, W, H, bind=False)
        both(rt.ERR_INVALID_OPERATION, sel=sel(shape=model.MASK), mask=foreign, tag="foreign mask")
        # unbound slots, on a context that has never made a call: the counts stay 0
        for bound in ((), (0,), (6,), (7,), (0, 6), (0, 7), (6, 7)):
            keep = []
            for s in bound:
                data = np.zeros(16, np.uint32) if s == 0 else cases.FLOATS["unit"] if s == 6 else cases.ints_of(3)
                keep.append(rt.VertexBufferObject(other, data))
                other.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, keep[-1])
            assert extract(other, view, good, None, None, 0)[0] == rt.ERR_INCOMPLETE, bound
            assert edit(other, rt.REGION_CLEAR, view, good, None, None)[0] == rt.ERR_INCOMPLETE, bound
            assert other.screen_counts() == (0, 0, 0, 0)
            for s in bound:
                other.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, None)
    finally:
        other.close()
    # max_depth outside 1..10 and a scale that is not positive and finite
    for d in (0, 11, -1):
        bad = rt.VertexBufferObject(ctx, np.array([d, 64, 64], np.int32))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, bad)
        both(INV, tag=("depth", d))
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ctx._keep[2])
    for s in (0.0, -1.0, np.inf, np.nan):
        f = cases.FLOATS["unit"].copy()
        f[4] = s
        bad = rt.VertexBufferObject(ctx, f)
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 6, bad)
        both(INV, tag=("scale", s))
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 6, ctx._keep6)
    # all of it left the context working
    rc, got, k = extract(ctx, view, sel(shape=model.MASK), None, mask, len(V))
    assert rc == 0 and got.tobytes() == lst.tobytes() and ctx.screen_counts() == counts


def test_counts_are_zero_before_any_call_and_on_an_empty_tree():
    c = rt.Context(0)
    try:
        assert c.screen_counts() == (0, 0, 0, 0)
        depth = 3
        cells = rt.VertexBufferObject(c, np.zeros(16, np.uint32))
        c.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, cells)
        fl = rt.VertexBufferObject(c, cases.FLOATS["unit"])
        c.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 6, fl)
        ints = rt.VertexBufferObject(c, cases.ints_of(depth))
        c.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
        view = cases.look((0.5, 0.5, -1.0), 0.0, 0.0, 0.5, 0.5, 8, 8)
        got = c.octree_extract_screen(c_view(view), rect=(0, 0, 7, 7))
        assert got.shape == (0, 4) and c.screen_counts() == (0, 0, 0, 0)
        assert c.octree_edit_screen(rt.REGION_CLEAR, c_view(view), rect=(0, 0, 7, 7)) == 1
        assert not cells.read(np.uint32).any() and c.screen_counts() == (0, 0, 0, 0)
    finally:
        c.close()


# ---- 5. a two-member context, and the renderer ------------------------------------------------------------------------------------------
def test_two_members_edit_both_replicas_and_refuse_a_mask():
    """A two-share context shards the frame over its members, so the frame after the edit shows every replica's cells: it must be, bit
    for bit, the single-device frame after the same edit.  A MASK edit is refused with nothing changed on either."""
    scene = host.Scene.config(2)
    full = sum(8 ** l for l in range(scene.max_depth))          # no tree of this depth has more cells: any result fits
    scene.blobs[0] = padded(np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), 64 * full)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            first = r.render()
            V = r.ctx.octree_extract()
            rect = (30, 20, 60, 45)
            picked = r.select_through(rect=rect, max_distance=0.5)
            counts = r.ctx.screen_counts()
            cells0 = r.vbos[0].read(np.uint32)
            if devices:
                assert rt.lib().tdt_ctx_device_count(r.ctx.h) == 2
                mask = rt.Texture.new_2d(r.ctx, 96, 64, bind=False)
                with pytest.raises(rt.TdtError) as e:
                    r.ctx.octree_edit_screen(rt.REGION_CLEAR, r.shader.view(), mask=mask)
                assert e.value.code == rt.ERR_INVALID_OPERATION
                assert np.array_equal(r.vbos[0].read(np.uint32), cells0) and r.ctx.screen_counts() == counts
                assert np.array_equal(r.render().view(np.uint32), first.view(np.uint32))
                assert len(r.ctx.octree_extract_screen(r.shader.view(), mask=mask)) == 0          # (an all-zero mask; extracts answer from member 0)
                r.select_through(rect=rect, max_distance=0.5)
            nc = r.ctx.octree_edit_screen(rt.REGION_PAINT, r.shader.view(), rect=rect, max_distance=0.5, paint_material=3)
            outs.append((nc, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), picked, np.array(counts), V))
        finally:
            r.close()
    one, two = outs
    for k, (a, b) in enumerate(zip(one, two)):
        if isinstance(a, np.ndarray) and a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), k
    nc, cells, frame, after, picked, counts, V = two
    assert 0 < len(picked) < len(V) and counts[3] == len(picked)
    keys = set(map(tuple, picked[:, :3]))
    hit = np.array([tuple(v) in keys for v in after[:, :3]])
    assert len(after) == len(V) and (after[hit, 3] == 4).all() and np.array_equal(after[~hit], V[~hit])
    assert not np.array_equal(frame.view(np.uint32), first.view(np.uint32))
    # the list is the model's, through the renderer's own view
    fl, ints = np.asarray(scene.blobs[6], F).ravel(), np.asarray(scene.blobs[7], np.int32).ravel()
    view = model_view(cam)
    want, wc = model.extract(V, fl, ints, view, model.sel_of(model.RECT, rect=(30, 20, 60, 45), max_distance=0.5))
    assert picked.tobytes() == want.tobytes() and tuple(counts) == wc


def model_view(cam):
    from reproject_model import view_of
    return view_of(list(cam.origin), list(cam.lower_left_corner), list(cam.horizontal), list(cam.vertical), cam.image_width, cam.image_height)


# ---- 6. the demo binary ------------------------------------------------------------------------------------------------------------------
def test_demo_lasso_preview_and_select_through_edit(tmp_path):
    """tdt_demo --lasso .. --preview draws Renderer.select_through's list over the frame; --select-through .. --op clear leaves the frame
    of Context.octree_edit_screen; both print the call's counts."""
    import re

    from test_gpu_select import _bits, _demo, _demo_renderer
    lasso = [(8, 6), (60, 10), (40, 44)]
    frame, stdout = _demo(tmp_path, "--lasso", ";".join("%d,%d" % p for p in lasso), "--window", "--preview")
    r = _demo_renderer()
    try:
        voxels = r.select_through(polygon=np.array(lasso, np.int32), window=True)
        counts = r.ctx.screen_counts()
        want, _ = r.render_overlay(voxels)
    finally:
        r.close()
    assert 0 < len(voxels) == counts[3] < counts[0]
    assert "select-through voxels %d on-screen %d in-shape %d selected %d list %d" % (*counts, len(voxels)) in stdout, stdout
    assert re.search(r"preview voxels %d pixels" % len(voxels), stdout) and _bits(frame).tobytes() == _bits(want).tobytes()
    frame, stdout = _demo(tmp_path, "--select-through", "16,12,47,35", "--only-material", "1", "--max-distance", "0.625", "--op", "clear")
    r = _demo_renderer()
    try:
        cells = r.ctx.octree_edit_screen(rt.REGION_CLEAR, r.shader.view(), rect=(16, 12, 47, 35), material=1, max_distance=0.625)
        counts = r.ctx.screen_counts()
        want = r.render()
    finally:
        r.close()
    assert 0 < counts[3] < 10                                     # (the rectangle holds 10 voxels of material 1; the distance cuts them)
    assert "select-through op clear voxels %d on-screen %d in-shape %d selected %d cells %d" % (*counts, cells) in stdout, stdout
    assert _bits(frame).tobytes() == _bits(want).tobytes()
