"""Screen-space selection on the GPU (csrc/tdt_select.hip) against tests/select_model.py: a voxel-id image is, byte for byte,
host.pick_grid_voxel of a pick of every pixel; an overlay and an extraction are the model's bytes on synthetic id images of every
tile shape; a flood selection and a marquee edit round-trip through a renderer; every error returns its code and writes nothing; a
two-member context gives the single-device bytes; and tdt_demo --preview / --select-rect do what the Renderer's calls do."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import select_model as model
import tree_model
from image_util import SIZES, _all_pixels, _bits, _raises, _wrapped
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
COVER = (64, 64)                                      # a dispatch whose 32x32 work-groups cover all of 64x48: render(*COVER)
OUTSIDE, INSIDE = ((0.0, 0.2, 0.9), 0.0, -8.0, 90.0), ((0.0, -0.1, -0.3), 0.0, 0.0, 90.0)
VAL, OP, INC = rt.ERR_INVALID_VALUE, rt.ERR_INVALID_OPERATION, rt.ERR_INCOMPLETE


def _cam(origin, yaw, pitch, fov, w=W, h=H, spp=2, bounce=3):
    c = host.Camera(fov, w, aspect_ratio=F(w) / F(h), origin=origin, viewport_height=2.0, samples_per_pixel=spp, max_bounce=bounce)
    if yaw:
        c.turn_yaw(yaw)
    if pitch:
        c.turn_pitch(pitch)
    return c.uniforms()


def _box(lo, hi, m):
    g = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([g, np.full((len(g), 1), m)], 1)


def depth1_scene():
    """Three of the eight voxels of a one-level tree; the inside pose stands in the empty voxel (1, 0, 1)."""
    vox = np.array([[0, 0, 0, 1], [1, 1, 0, 2], [0, 1, 1, 3]], np.int64)
    return tree_model.scene_from_cells(tree_model.build_cells(vox, 1), 1, 1 << 16, host.Scene.config(1))


def depth10_scene():
    """A depth-10 tree in front of both poses: a wall most of whose voxels have bit 9 of every coordinate set (the key's top three
    bits), a block in the low octant, and loose voxels around the middle."""
    rng = np.random.default_rng(10)
    loose = np.unique(rng.integers(380, 650, (400, 3)), axis=0)
    parts = [_box((520, 440, 520), (900, 640, 528), 1), _box((300, 300, 200), (364, 332, 264), 3),
             np.concatenate([loose, rng.integers(1, 5, (len(loose), 1))], 1)]
    vox = np.concatenate(parts)
    _, first = np.unique(vox[:, :3], axis=0, return_index=True)
    cells = tree_model.build_cells(vox[np.sort(first)], 10)
    assert cells.size // 16 < 1 << 16
    return tree_model.scene_from_cells(cells, 10, 1 << 16, host.Scene.config(1))


SCENES = {
    "demo": host.Scene.demo,
    "config1": lambda: host.Scene.config(1),
    "terrain8": lambda: host.Scene.generate(host.SCENE_TERRAIN, 8, 1 << 20, 100, 0x9A1C4),
    "depth1": depth1_scene,
    "depth10": depth10_scene,
}


# ---- 1. ids equal pick -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", [OUTSIDE, INSIDE], ids=["outside", "inside"])
@pytest.mark.parametrize("name", list(SCENES))
def test_ids_are_pick_grid_voxel_of_a_pick(name, pose):
    scene = SCENES[name]()
    floats, ints = scene.blobs[6], scene.blobs[7]
    r = rt.Renderer(scene, _cam(*pose))
    try:
        before = r.render()
        states, top_keys = set(), False
        for w, h in ((W, H), (33, 17), (1, 1)):                      # (the camera stays 64 x 48: it defines the rays, not the image)
            tex = rt.Texture.new_2d(r.ctx, w, h, bind=False)
            xy = _all_pixels(w, h)
            for sample in (0, 3):
                hits = r.pick(xy, sample=sample).reshape(h, w)
                for place in (0, 1):
                    want = model.ids_from_hits(hits, floats, ints, place)
                    r.shader.dispatch_voxel_ids(tex, place, sample)
                    got = tex.read_voxel_ids()
                    assert got.tobytes() == want.tobytes(), (name, w, h, sample, place, int((got != want).sum()))
                    if (w, h) == (W, H):
                        states |= set(np.unique(got["state"]).tolist())
                        top_keys |= bool(((got["state"] == 1) & (got["key"] >> 27 == 7)).any())
        assert states == {0, 1}, states                               # some pixels have a voxel, some do not
        if name == "depth10":
            assert top_keys                                           # bit 9 of x, y and z: the key's bits 29, 28, 27
        assert r.render().tobytes() == before.tobytes()               # the image, the cost history and the carry were left alone
    finally:
        r.close()


# ---- 2. overlay and extract on synthetic id images -------------------------------------------------------------------------
def make_ids(w, h, pattern, seed):
    """(ids, member keys, other keys).  `random`: patches of 3x2 texels share a voxel out of eight, a fifth of the texels have
    none.  `seam`: the member voxels fill exactly the first 32x8 tile (clipped to the image), so the selection's border runs along
    both tile seams; around it other voxels and texels without one.  `borders`: members along all four borders of the image, a
    hole of other voxels and empty texels in the middle."""
    rng = np.random.default_rng(seed)
    keys = model.morton(*rng.choice(1024, (3, 8), replace=False))
    mem, other = keys[:3], keys[3:]
    ids = np.zeros((h, w), model.ID_DTYPE)
    blocks = lambda n: np.repeat(np.repeat(rng.integers(0, n, ((h + 1) // 2, (w + 2) // 3)), 2, 0), 3, 1)[:h, :w]  # noqa: E731
    if pattern == "random":
        ids["key"] = keys[blocks(8)]
        ids["state"] = rng.random((h, w)) < 0.8
    else:
        ids["key"] = other[blocks(5)]
        ids["state"] = rng.random((h, w)) < 0.7
        inside = np.zeros((h, w), bool)
        if pattern == "seam":
            inside[:8, :32] = True
        else:
            inside[:] = True
            inside[h // 3:h - h // 3, w // 3:w - w // 3] = h < 3 or w < 3
        ids["key"][inside] = mem[blocks(3)][inside]
        ids["state"][inside] = 1
    ids["key"][ids["state"] == 0] = 0
    ids["material"] = rng.integers(0, 6, (h, w))
    ids["t"] = rng.integers(0, 2 ** 31, (h, w))
    return ids, mem, other


def make_image(w, h, seed):
    """Colours with NaN texels of one payload and infinities of one sign among them."""
    rng = np.random.default_rng(seed + 1000)
    img = (rng.random((h, w, 4)) * 2).astype(F)
    special = rng.random((h, w, 4))
    img[special < 0.04] = F(np.nan)
    img[(special >= 0.04) & (special < 0.08)] = F(np.inf)
    img[(special >= 0.08) & (special < 0.10)] = F(-0.0)
    return img


def _voxels(keys, m=1):
    v = model.voxel_of(np.asarray(keys, np.uint32)).reshape(-1, 3)
    return np.concatenate([v, np.full((len(v), 1), m, np.int32)], 1).astype(np.int32)


def make_lists(mem, other, seed):
    """name -> list.  `off grid` holds voxels of OTHER keys moved off the grid by 1024 and -1: taken modulo 1024 they would select
    what must stay unselected.  The long lists pad the members with voxels drawn at random."""
    rng = np.random.default_rng(seed + 2000)
    members = _voxels(mem)
    off = _voxels(other)
    off[:, 0] += 1024
    neg = _voxels(other[:2])
    neg[:, 1] = -1
    pad = lambda n: np.concatenate([rng.integers(0, 1024, (n - len(members), 3)), rng.integers(0, 255, (n - len(members), 1))], 1).astype(np.int32)  # noqa: E731
    return {
        "empty": np.zeros((0, 4), np.int32),
        "one": members[:1],
        "duplicates": np.concatenate([members, members[::-1], members[1:2]]),
        "unsorted": members[np.argsort(-model.morton(*members[:, :3].T).astype(np.int64))],
        "off grid": np.concatenate([off[:2], members, neg, off[2:]]),
        "257": rng.permutation(np.concatenate([members, pad(257)])),
        "5000": rng.permutation(np.concatenate([members, pad(5003)])),
    }


def _same_overlay(got, want, member, what):
    """Byte for byte; only a NaN the arithmetic computed (a member pixel's r, g, b) may be any NaN: the header leaves its sign and
    payload open, and numpy and the device do differ in the sign of inf * 0."""
    differ = _bits(got) != _bits(want)
    loose = differ & np.isnan(got) & np.isnan(want) & member[..., None] & np.array([True, True, True, False])
    assert not (differ & ~loose).any(), (what, int((differ & ~loose).sum()))


def pattern_holds_what_it_is_meant_to(w, h, pattern, ids, img, lists):
    """By the model alone: member, edge, non-member and state == 0 pixels occur where the pattern is meant to have them (an image
    too small for a pattern is run all the same: 1x1 and 2x2, and `seam` inside one tile, where everything is a member)."""
    _, member, edge, _ = model.overlay(img, ids, lists["unsorted"], dict(fill=(0, 0, 0, 1), edge=(0, 0, 0, 1), edge_width=1, flags=0))
    others = ~member & (ids["state"] == 1)
    if w < 5 or h < 5:
        return
    if pattern == "random":
        assert member.any() and edge.any() and (member & ~edge).any() and others.any() and (ids["state"] == 0).any()
    elif pattern == "seam":
        assert member[:8, :32].all() and not member[8:].any() and not member[:, 32:].any()
        if h > 8:
            assert edge[7, :min(w, 32)].all() and not edge[:6, 1:min(w, 31)].any()
        if w > 32:
            assert edge[:min(h, 8), 31].all()
        if h > 8 or w > 32:
            assert others.any() and (ids["state"] == 0).any()
    else:
        assert member[0].all() and member[-1].all() and member[:, 0].all() and member[:, -1].all()
        assert edge.any() and others.any() and (ids["state"] == 0).any() and (h < 7 or (member & ~edge).any())


CASES = [(w, h, p) for (w, h) in SIZES + [(32, 8), (31, 7), (33, 9)] for p in ("random", "seam", "borders")]


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context()
    yield c
    c.close()


@pytest.mark.parametrize("w,h,pattern", CASES, ids=[f"{w}x{h}-{p}" for w, h, p in CASES])
def test_overlay_is_the_model(ctx, w, h, pattern):
    import torch
    seed = w * 131 + h * 7 + len(pattern)
    ids, mem, other = make_ids(w, h, pattern, seed)
    img = make_image(w, h, seed)
    lists = make_lists(mem, other, seed)
    pattern_holds_what_it_is_meant_to(w, h, pattern, ids, img, lists)
    i_t, i_tex = _wrapped(ctx, ids)
    p_t, p_tex = _wrapped(ctx, img)
    pristine = p_t.clone()
    combo = 0
    for ew in (0, 1, 2, 4):
        for flags in (0, rt.OVERLAY_VOXEL_EDGES):
            for lname, voxels in lists.items():
                a = (0.0, 0.35, 1.0)[combo % 3]
                combo += 1
                style = dict(fill=(1.0, 0.6, 0.0, a), edge=(0.25, 1.5, 3.0, (1.0, 0.0, 0.35)[combo % 3]), edge_width=ew, flags=flags)
                want, member, edge, counts = model.overlay(img, ids, voxels, style)
                p_t.copy_(pristine)
                torch.cuda.synchronize()
                p_tex.overlay(i_tex, voxels, style["fill"], style["edge"], ew, bool(flags))
                got = p_tex.read()
                what = (w, h, pattern, ew, flags, lname, a)
                _same_overlay(got, want, member, what)
                assert ctx.overlay_counts() == counts, what
                if lname == "empty":
                    assert _bits(got).tobytes() == _bits(img).tobytes() and counts[2] == 0
                assert i_tex.read_voxel_ids().tobytes() == ids.tobytes(), what


@pytest.mark.parametrize("w,h", SIZES + [(33, 9)], ids=[f"{w}x{h}" for w, h in SIZES + [(33, 9)]])
def test_extract_is_the_model(ctx, w, h):
    ids, _, _ = make_ids(w, h, "random", w * 17 + h)
    i_t, tex = _wrapped(ctx, ids)
    whole = model.extract_voxels(ids)
    if w * h > 100:
        sel = ids[ids["state"] == 1]
        assert len(np.unique(sel[["key", "material"]])) > len(np.unique(sel["key"])) == len(whole)     # a key with several materials: the last wins
    ys, xs = np.nonzero(ids["state"] == 1)
    rects = [None, (0, 0, w - 1, h - 1), (-7, -3, w // 2, h + 5), (w // 2, h // 2, 10 * w, 10 * h), (w // 3, h // 3, w // 3, h // 3),
             (3, 0, 2, h - 1), (0, 2, w - 1, 1), (w, 0, w + 5, 5), (-9, -9, -1, -1)]
    if len(xs):
        rects.append((int(xs[0]), int(ys[0]), int(xs[0]), int(ys[0])))                                  # one pixel that has a voxel
    for rect in rects:
        want = model.extract_voxels(ids, rect)
        got = tex.extract_voxels(rect)
        assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (w, h, rect)
    assert len(model.extract_voxels(ids, (3, 0, 2, h - 1))) == 0 and len(model.extract_voxels(ids, (w, 0, w + 5, 5))) == 0
    # count only, and a capacity one short: INVALID_VALUE, the count still set, nothing written
    L, n = rt.lib(), ctypes.c_size_t(77)
    assert L.tdt_image_extract_voxels(tex.h, None, None, 0, ctypes.byref(n)) == rt.OK and n.value == len(whole)
    if len(whole):
        out = np.full((len(whole), 4), -5, np.int32)
        n = ctypes.c_size_t(77)
        assert L.tdt_image_extract_voxels(tex.h, None, out.ctypes.data, len(whole) - 1, ctypes.byref(n)) == VAL
        assert n.value == len(whole) and (out == -5).all()
        # a selected texel with material 254 is refused, outside the rectangle it does not matter
        bad = ids.copy()
        y, x = int(ys[-1]), int(xs[-1])
        bad["material"][y, x] = 254
        b_t, b_tex = _wrapped(ctx, bad)
        n = ctypes.c_size_t(77)
        assert L.tdt_image_extract_voxels(b_tex.h, None, out.ctypes.data, len(whole), ctypes.byref(n)) == VAL and (out == -5).all()
        if x > 0:
            assert (b_tex.extract_voxels((0, 0, x - 1, h - 1)) == model.extract_voxels(bad, (0, 0, x - 1, h - 1))).all()
    assert tex.read_voxel_ids().tobytes() == ids.tobytes()


# ---- 3. round trips on a renderer ------------------------------------------------------------------------------------------
def test_a_flood_selection_tints_exactly_the_pixels_that_pick_it():
    scene = host.Scene.config(1)
    r = rt.Renderer(scene, _cam(*OUTSIDE))
    try:
        xy = _all_pixels(W, H)
        hits = r.pick(xy).reshape(H, W)
        ids0 = model.ids_from_hits(hits, scene.blobs[6], scene.blobs[7], 0)
        ys, xs = np.nonzero(ids0["state"] == 1)
        y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
        seed = host.pick_grid_voxel(hits[y, x], scene, 0)
        voxels = r.ctx.octree_extract_connected(seeds=[seed], match=rt.MATCH_MATERIAL)
        assert len(voxels) >= 1
        plain = r.render(*COVER)
        frame, ids = r.render_overlay(voxels, fill=(2.0, 3.0, 4.0, 1.0), edge_width=0, width=COVER[0], height=COVER[1])
        assert ids.tobytes() == ids0.tobytes()
        member = model.membership(ids0, voxels)
        assert member[y, x] and member.any() and not member.all()
        tinted = (frame[..., :3] == np.array([2.0, 3.0, 4.0], F)).all(-1)
        assert (tinted == member).all()
        assert _bits(frame[~member]).tobytes() == _bits(plain[~member]).tobytes() and (_bits(frame[..., 3]) == _bits(plain[..., 3])).all()
        assert r.ctx.overlay_counts() == (W * H, int((ids0["state"] == 1).sum()), int(member.sum()), 0)
        # the default style: an outline of one pixel, the model's bytes
        frame, _ = r.render_overlay(voxels, width=COVER[0], height=COVER[1])
        want, _, edge, counts = model.overlay(plain, ids0, voxels, dict(fill=(1, .6, 0, .35), edge=(1, .6, 0, 1), edge_width=1, flags=0))
        assert _bits(frame).tobytes() == _bits(want).tobytes() and edge.any() and r.ctx.overlay_counts() == counts
    finally:
        r.close()


def test_a_marquee_clear_removes_what_the_rectangle_showed():
    scene = host.Scene.config(1)
    r = rt.Renderer(scene, _cam(*OUTSIDE))
    try:
        rect = (16, 12, 47, 35)
        before = r.ctx.octree_census()["voxels"]
        hits = r.pick(_all_pixels(W, H)).reshape(H, W)
        want = model.extract_voxels(model.ids_from_hits(hits, scene.blobs[6], scene.blobs[7], 0), rect)
        removed = r.select_rect(rect)
        assert len(removed) > 0 and (removed == want).all()
        r.ctx.octree_edit_voxels(rt.REGION_CLEAR, removed)
        assert r.ctx.octree_census()["voxels"] == before - len(removed)
        tex = rt.Texture.new_2d(r.ctx, W, H, bind=False)
        r.shader.dispatch_voxel_ids(tex)
        ids = tex.read_voxel_ids()
        gone = model.morton(*removed[:, :3].T)
        assert (ids["state"] == 1).any() and not np.isin(ids["key"][ids["state"] == 1], gone).any()
        # place 1 over the same rectangle now: cells that are empty, painted back in they grow the tree by their number
        front = r.select_rect(rect, place=1)
        assert len(front) > 0
        r.ctx.octree_edit_voxels(rt.REGION_FILL, front)
        assert r.ctx.octree_census()["voxels"] == before - len(removed) + len(front)
    finally:
        r.close()


# ---- 4. errors and other contexts ------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(1)
    r = rt.Renderer(scene, _cam(*INSIDE))
    other = rt.Context()
    try:
        ids, mem, _ = make_ids(33, 17, "random", 5)
        img = make_image(33, 17, 5)
        i_t, i_tex = _wrapped(r.ctx, ids)
        p_t, p_tex = _wrapped(r.ctx, img)
        s_t, s_tex = _wrapped(r.ctx, img[:16, :32])                   # another size
        o_t, o_tex = _wrapped(other, img)                             # another context
        vox = np.ascontiguousarray(_voxels(mem))
        style = rt.Overlay((ctypes.c_float * 4)(1, 0, 0, 1), (ctypes.c_float * 4)(0, 1, 0, 1), 1, 0)
        p_tex.overlay(i_tex, vox, (1, 0, 0, 1))
        done, counts = p_tex.read(), r.ctx.overlay_counts()
        assert counts[2] > 0

        def unchanged():
            assert _bits(p_tex.read()).tobytes() == _bits(done).tobytes() and i_tex.read_voxel_ids().tobytes() == ids.tobytes()
            assert r.ctx.overlay_counts() == counts

        # tdt_dispatch_voxel_ids
        assert L.tdt_dispatch_voxel_ids(None, i_tex.h, 0, 0) == VAL
        assert L.tdt_dispatch_voxel_ids(r.shader.h, None, 0, 0) == VAL
        for place, sample in ((2, 0), (-1, 0), (0, -1)):
            assert L.tdt_dispatch_voxel_ids(r.shader.h, i_tex.h, place, sample) == VAL
        assert L.tdt_dispatch_voxel_ids(r.shader.h, o_tex.h, 0, 0) == OP
        update = rt.ComputeShader(r.ctx, rt.PROGRAM_OCTREE_UPDATE)
        assert L.tdt_dispatch_voxel_ids(update.h, i_tex.h, 0, 0) == OP
        r.shader.set_partition(1, 2)
        assert L.tdt_dispatch_voxel_ids(r.shader.h, i_tex.h, 0, 0) == OP
        r.shader.set_partition(0, 1)
        bare = rt.ComputeShader(other)
        assert L.tdt_dispatch_voxel_ids(bare.h, o_tex.h, 0, 0) == INC                     # slots 0, 6, 7 unbound
        unchanged()
        # tdt_image_overlay
        n = len(vox)
        assert L.tdt_image_overlay(None, i_tex.h, vox.ctypes.data, n, ctypes.byref(style)) == VAL
        assert L.tdt_image_overlay(p_tex.h, None, vox.ctypes.data, n, ctypes.byref(style)) == VAL
        assert L.tdt_image_overlay(p_tex.h, i_tex.h, vox.ctypes.data, n, None) == VAL
        assert L.tdt_image_overlay(p_tex.h, i_tex.h, None, n, ctypes.byref(style)) == VAL
        assert L.tdt_image_overlay(p_tex.h, i_tex.h, vox.ctypes.data, (1 << 26) + 1, ctypes.byref(style)) == VAL
        for ew, flags in ((-1, 0), (5, 0), (1, 2), (1, 0x80000000)):
            bad = rt.Overlay((ctypes.c_float * 4)(1, 0, 0, 1), (ctypes.c_float * 4)(0, 1, 0, 1), ew, flags)
            assert L.tdt_image_overlay(p_tex.h, i_tex.h, vox.ctypes.data, n, ctypes.byref(bad)) == VAL
        assert L.tdt_image_overlay(p_tex.h, s_tex.h, vox.ctypes.data, n, ctypes.byref(style)) == VAL      # sizes differ
        assert L.tdt_image_overlay(p_tex.h, p_tex.h, vox.ctypes.data, n, ctypes.byref(style)) == VAL      # the same image
        assert L.tdt_image_overlay(p_tex.h, o_tex.h, vox.ctypes.data, n, ctypes.byref(style)) == OP
        unchanged()
        # tdt_image_extract_voxels, tdt_debug_overlay_counts
        k = ctypes.c_size_t(0)
        assert L.tdt_image_extract_voxels(None, None, None, 0, ctypes.byref(k)) == VAL
        assert L.tdt_image_extract_voxels(i_tex.h, None, None, 0, None) == VAL
        assert L.tdt_debug_overlay_counts(None, (ctypes.c_uint64 * 4)()) == VAL and L.tdt_debug_overlay_counts(r.ctx.h, None) == VAL
        assert other.overlay_counts() == (0, 0, 0, 0)                                     # before any call
        unchanged()
    finally:
        other.close()
        r.close()


@pytest.mark.parametrize("what,value", [("depth", 11), ("depth", 0), ("scale", 0.0), ("scale", -1.0), ("scale", float("inf")), ("scale", float("nan"))])
def test_a_tree_the_key_cannot_hold_is_refused(what, value):
    like = host.Scene.config(1)
    blobs = {k: v.copy() for k, v in like.blobs.items()}
    if what == "depth":
        blobs[7][0] = value
    else:
        blobs[6][4] = value
    r = rt.Renderer(host.Scene(blobs, like.counts, "refused"), _cam(*INSIDE))
    try:
        tex = rt.Texture.new_2d(r.ctx, 8, 8, bind=False)
        tex.clear()
        _raises(VAL, r.shader.dispatch_voxel_ids, tex)
        assert not _bits(tex.read()).any()
    finally:
        r.close()


def test_two_members_give_the_single_device_bytes():
    scene, cam = host.Scene.config(1), _cam(*INSIDE)
    one = rt.Renderer(scene, cam)
    try:
        tex = rt.Texture.new_2d(one.ctx, W, H, bind=False)
        one.shader.dispatch_voxel_ids(tex, 1, 3)
        ids1 = tex.read_voxel_ids()
        voxels = tex.extract_voxels((5, 5, 40, 30))                   # (empty cells in front of faces)
        shown = one.select_rect((5, 5, 40, 30))                       # (the voxels behind them: what place 0 ids can show)
        frame1, ids0 = one.render_overlay(shown, place=0, voxel_edges=True)
        counts = one.ctx.overlay_counts()
    finally:
        one.close()
    r = rt.Renderer(scene, cam, devices=[0, 0])
    try:
        tex = rt.Texture.new_2d(r.ctx, W, H, bind=False)
        r.shader.dispatch_voxel_ids(tex, 1, 3)
        assert tex.read_voxel_ids().tobytes() == ids1.tobytes()
        assert (tex.extract_voxels((5, 5, 40, 30)) == voxels).all() and len(voxels) > 0
        assert (r.select_rect((5, 5, 40, 30)) == shown).all()
        frame, ids = r.render_overlay(shown, place=0, voxel_edges=True)
        assert ids.tobytes() == ids0.tobytes() and _bits(frame).tobytes() == _bits(frame1).tobytes()
        assert r.ctx.overlay_counts() == counts and counts[2] > 0 and counts[3] > 0
    finally:
        r.close()


# ---- 5. the demo binary ----------------------------------------------------------------------------------------------------
def _demo(tmp_path, *args):
    from tdt4230_project_raytracing_amd import build
    out = str(tmp_path / "frame.pfm")
    run = subprocess.run([build.build_demo(), "--config", "1", "--size", f"{W}x{H}", *args, "--out", out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    with open(out, "rb") as fh:
        assert fh.readline().strip() == b"PF4" and fh.readline().split() == [str(W).encode(), str(H).encode()]
        fh.readline()
        return np.frombuffer(fh.read(), "<f4").reshape(H, W, 4), run.stdout


def _demo_renderer():
    c = host.Camera(90.0, W, aspect_ratio=F(W) / F(H), origin=[0.0, -0.1, -0.3], viewport_height=2.0, samples_per_pixel=4, max_bounce=6,
                    turn_rate=0.05)
    return rt.Renderer(host.Scene.config(1), c.uniforms())


def test_demo_preview_writes_render_overlays_frame(tmp_path):
    frame, stdout = _demo(tmp_path, "--pick", "32,24", "--flood", "clear", "--match", "material", "--preview")
    r = _demo_renderer()
    try:
        before = r.ctx.octree_census()["voxels"]
        hit = r.pick([[32, 24]])[0]
        voxels = r.ctx.octree_extract_connected(seeds=[host.pick_grid_voxel(hit, host.Scene.config(1), 0)], match=rt.MATCH_MATERIAL)
        want, _ = r.render_overlay(voxels)
        counts = r.ctx.overlay_counts()
        assert r.ctx.octree_census()["voxels"] == before
    finally:
        r.close()
    assert _bits(frame).tobytes() == _bits(want).tobytes()
    m = re.search(r"preview voxels (\d+) pixels (\d+) with-voxel (\d+) member (\d+) edge (\d+)", stdout)
    assert m and tuple(int(v) for v in m.groups()) == (len(voxels),) + counts and counts[2] > 0 and counts[3] > 0, stdout
    # a box: the tree's voxels inside it
    frame, stdout = _demo(tmp_path, "--box", "0,0,0,7,3,7", "--op", "clear", "--preview")
    r = _demo_renderer()
    try:
        voxels = r.ctx.octree_extract_region(rt.box((0, 0, 0), (7, 3, 7)))
        want, _ = r.render_overlay(voxels)
    finally:
        r.close()
    assert _bits(frame).tobytes() == _bits(want).tobytes() and f"preview box voxels {len(voxels)}" in stdout


def test_demo_select_rect_applies_select_rects_edit(tmp_path):
    frame, stdout = _demo(tmp_path, "--select-rect", "16,12,47,35", "--op", "clear")
    r = _demo_renderer()
    try:
        voxels = r.select_rect((16, 12, 47, 35))
        cells = r.ctx.octree_edit_voxels(rt.REGION_CLEAR, voxels)
        want = r.render()
    finally:
        r.close()
    assert f"select-rect 16,12,47,35 op clear voxels {len(voxels)} cells {cells}" in stdout and len(voxels) > 0
    assert _bits(frame).tobytes() == _bits(want).tobytes()
