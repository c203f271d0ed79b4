"""Temporal reprojection on the GPU (csrc/tdt_reproject.hip): the history, the mean and the counts are the bytes of the numpy model
(tests/reproject_model.py) on real frames of moving cameras and on hand-made data; Renderer.render_temporal is the chain
accumulate, reproject, (denoise,) resolve frame after frame, also across the wrap of its sample index; a static camera's error
falls as the theory says; a multi-device context gives the single-device bytes; errors write nothing; tdt_demo --temporal turns
by degrees and writes render_temporal's frame.

The primary rays the model is given are pick's (return_rays=True): nothing here restates the sampler.

A note on the pose pairs.  A camera that moves along a direction inside its own frustum without turning sees nothing new: every
point it sees now lay inside the old frustum too (X - A = (X - B) + (B - A) is a sum of two vectors of one convex cone), so a plain
move forward can never reject a pixel as off-screen.  The forward pair here is therefore a walk forward with the camera looking
down more steeply than half its vertical field of view — the heading is outside the frustum and floor enters at the top."""
import ctypes

import numpy as np
import pytest

import denoise_model
import reproject_model as model
from image_util import INSIDE_TURNED, _all_pixels, _bits, _wrapped
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
SPP = 4


def _cam(origin, yaw, pitch, fov, w=W, h=H, spp=SPP, bounce=6):
    c = host.Camera(fov, w, aspect_ratio=np.float32(w) / np.float32(h), origin=origin, viewport_height=2.0, samples_per_pixel=spp,
                    max_bounce=bounce)
    if yaw:
        c.turn_yaw(yaw)
    if pitch:
        c.turn_pitch(pitch)
    return c.uniforms()


def _units(degrees):
    """An angle in the units of turn_yaw / turn_pitch of a camera with the default turn_rate."""
    return float(np.radians(degrees)) / (2.0 * 0.025)


def _cover(w, h):
    """A dispatch whose 32x32 work-groups cover all of w x h."""
    return -(-w // 32) * 32, -(-h // 32) * 32


def _same(got, want, what):
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


# (origin, yaw, pitch, fov) of the earlier and of the current frame.  fov is in degrees; yaw and pitch are NOT: they are the
# arguments of host.Camera.turn_yaw / turn_pitch, which rotate by 2 * angle * turn_rate radians, 2.865 degrees per unit at the
# default turn_rate of 0.025 (_units converts).  So config1's yaw pair (135 -> 139) turns 11.5 degrees, the demo's (0 -> 1) 2.9
# degrees, and the sequence test below 5.7 degrees per frame; the forward pairs look down by 60 degrees.
# config1's voxels are 1/8 wide and many pixels of a 64x48 frame each.  The demo scene's are 1/1024 wide: from across the scene a pixel covers several of them, two jitters of ONE pixel land
# on different faces, and the identical pose finds 16 % of its keyed pixels again (29 of 187 from (0, 0.2, 0.9), measured) — that is
# what nearest-texel history gives on sub-pixel geometry, and DESIGN.md says so.  Its pairs here therefore look at the block of
# voxels in the octant x, y < 0, z < -0.5 from 0.05 away through a 3 degree lens, where a voxel is about twenty pixels wide.
CLOSE_UP = ((-0.2503, -0.2497, -0.45), 0.0, 0.0, 3.0)
PAIRS = {
    "config1": {
        "yaw": (INSIDE_TURNED, ((0.1, 0.05, -0.6), 139.0, 10.0, 70.0)),
        "sideways": (((0.0, -0.1, -0.3), 0.0, 0.0, 90.0), ((0.08, -0.1, -0.3), 0.0, 0.0, 90.0)),
        "forward": (((0.0, 0.7, -0.5), 0.0, _units(-60.0), 50.0), ((0.0, 0.7, -0.55), 0.0, _units(-60.0), 50.0)),
        "identical": (INSIDE_TURNED, INSIDE_TURNED),
    },
    "demo": {
        "yaw": (CLOSE_UP, ((-0.2503, -0.2497, -0.45), 1.0, 0.0, 3.0)),
        "sideways": (CLOSE_UP, ((-0.24925, -0.2497, -0.45), 0.0, 0.0, 3.0)),
        "forward": (((-0.2503, 0.05, -0.7503), 0.0, _units(-60.0), 3.0), ((-0.2503, 0.05, -0.75135), 0.0, _units(-60.0), 3.0)),
        "identical": (CLOSE_UP, CLOSE_UP),
    },
}


def _scene(name):
    return host.Scene.demo() if name == "demo" else host.Scene.config(1)


@pytest.fixture(scope="module")
def renderers():
    made = {}

    def get(name):
        if name not in made:
            made[name] = rt.Renderer(_scene(name), _cam(*INSIDE_TURNED))
        return made[name]
    yield get
    for r in made.values():
        r.close()


def gpu_frame(r, cam, sample, prev=None, max_samples=64.0, mean="own"):
    """One frame of cam's size on r's context, in textures of its own: the running sums of samples [sample, sample + spp), the guide
    of `sample`, pick's rays, and tdt_image_reproject over them (prev: a frame this function returned, or None).  mean: "own" (a
    texture of its own), "sums" (in place) or None."""
    w, h, spp = cam.image_width, cam.image_height, cam.samples_per_pixel
    rt.initial_uniforms(cam, r.shader.program)
    f = {"w": w, "h": h, "spp": spp, "sample": sample}
    f["sums_tex"] = rt.Texture.new_2d(r.ctx, w, h)                    # (bound)
    if sample:
        f["sums_tex"].clear()
    r.shader.dispatch_accumulate(*_cover(w, h), 1, sample, spp)
    f["sums"] = f["sums_tex"].read()
    f["guide_tex"] = rt.Texture.new_2d(r.ctx, w, h, bind=False)
    r.shader.dispatch_guide(f["guide_tex"], sample=sample)
    f["guide"] = f["guide_tex"].read_guide()
    f["rays"] = r.pick(_all_pixels(w, h), sample=sample, return_rays=True)[1].reshape(h, w, 6)
    f["hist_tex"] = rt.Texture.new_2d(r.ctx, w, h, bind=False)
    mean_tex = {"own": rt.Texture.new_2d(r.ctx, w, h, bind=False), "sums": f["sums_tex"], None: None}[mean]
    f["sums_tex"].reproject(r.shader, sample, f["guide_tex"], spp, None if prev is None else (prev["view"], prev["guide_tex"], prev["hist_tex"]),
                            max_samples, hist_out=f["hist_tex"], mean_out=mean_tex)
    f["counts"] = r.ctx.reproject_counts()
    f["hist"] = f["hist_tex"].read()
    f["mean"] = mean_tex.read() if mean_tex is not None else None
    f["view"] = r.shader.view()
    if mean != "sums":
        _same(f["sums_tex"].read(), f["sums"], "the sums are only read")
    _same(f["guide_tex"].read_guide(), f["guide"], "the guide is only read")
    return f


def model_frame(f, prev=None, max_samples=64.0):
    if prev is None:
        return model.reproject(f["rays"], f["guide"], f["sums"], f["spp"], None, None, None, max_samples)
    return model.reproject(f["rays"], f["guide"], f["sums"], f["spp"], model.view_from_ctypes(prev["view"]), prev["guide"], prev["hist"], max_samples)


def check_frame(f, prev, what, max_samples=64.0):
    hist, mean, _, found, counts = model_frame(f, prev, max_samples)
    print(f"{what}: keyed {counts[0]} found {counts[1]} rejected by key {counts[2]} off-screen {counts[3]} (GPU {f['counts']})")
    _same(f["hist"], hist, what + " history")
    if f["mean"] is not None:
        _same(f["mean"], mean, what + " mean")
    assert f["counts"] == counts, what
    return counts


# ---- 1. real frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ["yaw", "sideways", "forward", "identical"])
@pytest.mark.parametrize("name", ["config1", "demo"])
def test_real_frames_are_the_model_bit_for_bit(renderers, name, pair):
    r = renderers(name)
    a, b = PAIRS[name][pair]
    old = gpu_frame(r, _cam(*a), 0)
    first = check_frame(old, None, f"{name} {pair} first frame")
    assert first[0] > 0 and first[1:] == (0, 0, 0)
    u = _cam(*a)
    for field in ("origin", "lower_left_corner", "horizontal", "vertical"):
        assert list(getattr(old["view"], field)) == list(getattr(u, field)), field
    assert (old["view"].image_width, old["view"].image_height) == (W, H)
    cur = gpu_frame(r, _cam(*b), SPP, prev=old)
    keyed, found, by_key, off = model_frame(cur, old)[4]               # what the case claims, from the model alone
    print(f"{name} {pair}: the model finds {found} of {keyed} keyed pixels, rejects {by_key} by key and {off} as off-screen")
    if pair == "identical":
        assert found >= 0.9 * keyed, (found, keyed)
    else:
        assert found > 0 and by_key > 0 and off > 0, (keyed, found, by_key, off)
    assert found + by_key + off == keyed
    check_frame(cur, old, f"{name} {pair}")


@pytest.mark.parametrize("variant", ["33x17", "2x2", "40x30 into 64x48", "mean in place", "no mean"])
def test_sizes_and_outputs(renderers, variant):
    r = renderers("config1")
    a, b = PAIRS["config1"]["yaw"]
    size = {"33x17": (33, 17), "2x2": (2, 2)}.get(variant, (W, H))
    old_size = (40, 30) if variant.startswith("40x30") else size
    mean = {"mean in place": "sums", "no mean": None}.get(variant, "own")
    old = gpu_frame(r, _cam(*a, w=old_size[0], h=old_size[1]), 0, mean=mean)
    check_frame(old, None, variant + " first frame")
    cur = gpu_frame(r, _cam(*b, w=size[0], h=size[1]), SPP, prev=old, mean=mean)
    counts = check_frame(cur, old, variant)
    if variant != "2x2":
        assert counts[1] > 0


# ---- 2. hand-made data -----------------------------------------------------------------------------------------------------
def make_case(w, h, pw, ph, seed, cap):
    """Hand-made frames: guides of random patches of a few keys (two differ from the first by one ulp of `plane`, or only in
    `material`), single-texel islands and kind-0 holes, depths of 0.3..3; a history whose sample counts sit around the cap, at or
    below zero, or are NaN; colours with negatives, denormals, infinities of ONE sign and NaNs of one payload in the sums and in
    the history alike (inf - inf and an operation on two different NaNs leave sign and payload to the implementation)."""
    rng = np.random.default_rng(seed)
    base = F(0.3125)
    keys = [(14, 2, base), (14, 2, np.nextafter(base, F(1))), (14, 3, base), (16, 2, base)]

    def guide_of(gw, gh):
        g = np.zeros((gh, gw), denoise_model.GUIDE_DTYPE)
        which = np.zeros((gh, gw), np.int64)
        for _ in range(10):
            x0, y0 = int(rng.integers(0, gw)), int(rng.integers(0, gh))
            which[y0:y0 + int(rng.integers(1, gh // 2 + 2)), x0:x0 + int(rng.integers(1, gw // 2 + 2))] = int(rng.integers(0, len(keys)))
        for f, col in (("kind", 0), ("material", 1), ("plane", 2)):
            g[f] = np.array([k[col] for k in keys])[which]
        g["t"] = (0.3 + 2.7 * rng.random((gh, gw))).astype(F)
        flat = g.reshape(-1)
        spots = rng.permutation(gw * gh)
        n_i, n_h = max(1, gw * gh // 40), max(1, gw * gh // 12)
        for k, p in enumerate(spots[:n_i]):
            flat[p] = (20, 100 + k, F(k), flat[p]["t"])
        for p in spots[n_i:n_i + n_h]:
            flat[p] = (0, int(rng.integers(0, 4)), 0, flat[p]["t"])
        return g

    def colours(cw, ch):
        c = (rng.standard_normal((ch, cw, 4)) * 3).astype(F)
        special = rng.random((ch, cw, 4))
        c[special < 0.04] = F(1e-41)
        c[(special >= 0.04) & (special < 0.06)] = F(-3e-42)
        c[(special >= 0.06) & (special < 0.07)] = F(np.inf if seed % 2 else -np.inf)
        c[(special >= 0.07) & (special < 0.08)] = F(np.nan)
        return c

    cap = F(cap)
    counts = np.array([np.nextafter(cap, F(0)), cap, np.nextafter(cap, F(np.inf)), cap * F(3), F(0.5) if cap > 1 else F(1), F(0), F(-0.0), F(-1), F(np.nan)], F)
    prev_hist = colours(pw, ph)
    prev_hist[..., 3] = counts[rng.integers(0, len(counts), (ph, pw))]
    return {"guide": guide_of(w, h), "sums": colours(w, h), "prev_guide": guide_of(pw, ph), "prev_hist": prev_hist}


HAND_CUR = ((0.05, 0.1, 0.2), 20.0, -5.0, 80.0)
HAND_OLD = ((0.0, 0.1, 0.3), 16.0, -4.0, 80.0)


def run_case(r, case, w, h, cap, sample=5, spp=3):
    """tdt_image_reproject over the arrays of a hand-made case under r's HAND_CUR camera, the old view being HAND_OLD's:
    (hist, mean, counts, rays, old view)."""
    pw = case["prev_guide"].shape[1]
    rt.initial_uniforms(_cam(*HAND_OLD, w=pw + 3, h=case["prev_guide"].shape[0] + 2), r.shader.program)   # (the view's size is not the images')
    old_view = r.shader.view()
    rt.initial_uniforms(_cam(*HAND_CUR, w=w, h=h), r.shader.program)
    rays = r.pick(_all_pixels(w, h), sample=sample, return_rays=True)[1].reshape(h, w, 6)
    keep = [_wrapped(r.ctx, case[k]) for k in ("guide", "sums", "prev_guide", "prev_hist")]
    zeros = np.zeros((h, w, 4), F)
    hist, mean = _wrapped(r.ctx, zeros), _wrapped(r.ctx, zeros)
    keep[1][1].reproject(r.shader, sample, keep[0][1], spp, (old_view, keep[2][1], keep[3][1]), cap, hist_out=hist[1], mean_out=mean[1])
    counts = r.ctx.reproject_counts()
    out = hist[0].cpu().numpy(), mean[0].cpu().numpy(), counts
    for (t, _), k in zip(keep, ("guide", "sums", "prev_guide", "prev_hist")):
        assert _bits(t.cpu().numpy()).tobytes() == _bits(case[k]).tobytes(), k
    return out + (rays, old_view)


@pytest.mark.parametrize("cap", [1.0, 6.5, 1e30])
@pytest.mark.parametrize("w,h,pw,ph", [(64, 48, 64, 48), (33, 17, 50, 21), (16, 16, 7, 5)])
def test_hand_made_data_is_the_model_bit_for_bit(renderers, w, h, pw, ph, cap):
    r = renderers("config1")
    case = make_case(w, h, pw, ph, seed=w * 100 + pw + int(min(cap, 100)), cap=cap)
    hist, mean, counts, rays, old_view = run_case(r, case, w, h, cap)
    m_hist, m_mean, _, found, m_counts = model.reproject(rays, case["guide"], case["sums"], 3, model.view_from_ctypes(old_view), case["prev_guide"],
                                                         case["prev_hist"], cap)
    print(f"{w}x{h} from {pw}x{ph} cap {cap}: keyed, found, by key or count, off-screen = {m_counts}")
    assert m_counts[1] > 0 and m_counts[2] > 0 and m_counts[3] > 0 and m_counts[0] < w * h
    assert (m_hist[..., 3][found] == F(3) + F(cap)).any() or cap == F(1e30)       # the cap bit somewhere
    _same(hist, m_hist, "history")
    _same(mean, m_mean, "mean")
    assert counts == m_counts


# ---- 3. a sequence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 2])
def test_render_temporal_is_the_chain(oracle, passes):
    scene = host.Scene.config(1)
    o, yaw, pitch, fov = INSIDE_TURNED
    cams = [_cam(o, yaw + 2.0 * k, pitch, fov) for k in range(6)]
    cover = _cover(W, H)
    a, b = rt.Renderer(scene, cams[0]), rt.Renderer(scene, cams[0])
    try:
        plain = a.render(*cover)
        prev, frames = None, []
        for k, cam in enumerate(cams):
            got = a.render_temporal(*cover, cam=cam if k else None, denoise=passes, max_samples=10.0)
            f = gpu_frame(b, cam, k * SPP)                             # the GPU's own sums, guide and rays of frame k
            hist, mean, _, found, counts = model_frame(f, prev, 10.0)
            if k:
                assert counts[1] > 0 and counts[2] + counts[3] > 0
            if k >= 3:
                assert (hist[..., 3] == F(SPP) + F(10)).any()          # a history of 12 samples meets the cap of 10 in the fourth frame
            assert a.ctx.reproject_counts() == counts
            img = denoise_model.denoise(mean, f["guide"], passes) if passes else mean
            want = oracle.resolve(cam, img, 1, dispatch=cover)
            _same(got, want, f"frame {k}")
            frames.append(got)
            prev = {"view": f["view"], "guide": f["guide"], "hist": hist}
        assert frames[1].tobytes() != frames[0].tobytes()
        again = a.render_temporal(*cover, cam=cams[0], denoise=passes, max_samples=10.0, reset=True)
        _same(again, frames[0], "after a reset the frame is a first frame")
        assert a.render(*cover).tobytes() == plain.tobytes()          # the default path is what it was
    finally:
        a.close()
        b.close()
    fresh = rt.Renderer(scene, cams[0])
    try:
        assert fresh.render(*cover).tobytes() == plain.tobytes()
    finally:
        fresh.close()


def test_the_sample_index_wraps_and_the_history_goes_on(monkeypatch):
    """With the period set to two frames' samples, frame 2 traces samples [0, spp) again and still takes frame 1's history."""
    monkeypatch.setattr(rt, "TEMPORAL_SAMPLE_PERIOD", 2 * SPP)
    scene = host.Scene.config(1)
    cam = _cam(*INSIDE_TURNED)
    cover = _cover(W, H)
    a, b = rt.Renderer(scene, cam), rt.Renderer(scene, cam)
    try:
        prev = None
        for k, sample in enumerate((0, SPP, 0, SPP)):
            a.render_temporal(*cover)
            f = gpu_frame(b, cam, sample)
            hist, mean, _, found, counts = model_frame(f, prev)
            assert a.ctx.reproject_counts() == counts
            assert (counts[1] > 0) == (k > 0)
            _same(a.temporal["hist"][k & 1].read(), hist, f"frame {k} history")
            prev = {"view": f["view"], "guide": f["guide"], "hist": hist}
        assert hist[..., 3].max() == F(4 * SPP)                       # four frames' samples behind the best pixels
    finally:
        a.close()
        b.close()


# ---- 4. it helps -----------------------------------------------------------------------------------------------------------
def test_a_static_camera_gains_what_its_samples_promise():
    """8 temporal frames of 4 spp against one plain 4-spp frame, RMSE of the linear means over the keyed pixels against a 256-spp
    accumulate of the same view.  Below 1/sqrt(2) of the plain error is what two frames of independent samples would give; eight
    give about 0.35."""
    scene = host.Scene.config(1)
    cam = _cam(*INSIDE_TURNED)
    cover = _cover(W, H)
    r = rt.Renderer(scene, cam)
    try:
        r.shader.dispatch_accumulate(*cover, 1, 0, 256)
        ref = r.texture.read()[..., :3] / F(256)
        r.shader.dispatch_accumulate(*cover, 1, 0, SPP)
        plain = r.texture.read()[..., :3] / F(SPP)
        for k in range(8):
            r.render_temporal(*cover)
        h = r.temporal["hist"][7 & 1].read()
        keyed = r.temporal["guide"][7 & 1].read_guide()["kind"] != 0
        found = r.ctx.reproject_counts()
        temporal = h[..., :3] / h[..., 3:]
    finally:
        r.close()
    assert keyed.sum() > 200

    def rmse(img):
        return float(np.sqrt(np.mean((img[keyed].astype(np.float64) - ref[keyed]) ** 2)))
    e_plain, e_temporal = rmse(plain), rmse(temporal)
    print(f"RMSE over {int(keyed.sum())} keyed pixels: plain {e_plain:.5f}, temporal {e_temporal:.5f}, ratio {e_temporal / e_plain:.3f}; "
          f"last frame found {found[1]} of {found[0]}; mean history length {float(h[..., 3][keyed].mean()):.1f}")
    assert e_plain > 0
    assert e_temporal < e_plain / np.sqrt(2.0)


# ---- 5. several devices ----------------------------------------------------------------------------------------------------
def test_multi_device_context_runs_on_the_first_device(renderers):
    case = make_case(33, 17, 50, 21, seed=77, cap=6.5)
    one = run_case(renderers("config1"), case, 33, 17, 6.5)
    r = rt.Renderer(host.Scene.config(1), _cam(*INSIDE_TURNED), devices=[0, 0])
    try:
        two = run_case(r, case, 33, 17, 6.5)
        # tdt_image_clear refuses an image of a multi-device context (its running sums are in the members' tile buffers)
        marks = np.full((17, 33, 4), 7.0, F)
        t, tex = _wrapped(r.ctx, marks)
        assert rt.lib().tdt_image_clear(tex.h) == rt.ERR_INVALID_OPERATION
        assert rt.lib().tdt_image_clear(r.texture.h) == rt.ERR_INVALID_OPERATION
        r.ctx.finish()
        assert t.cpu().numpy().tobytes() == marks.tobytes()
    finally:
        r.close()
    assert one[2][1] > 0
    _same(two[0], one[0], "history")
    _same(two[1], one[1], "mean")
    assert two[2] == one[2]
    _same(two[3], one[3], "rays")


# ---- 6. errors -------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing_and_no_scene_is_needed():
    L = rt.lib()
    w, h, pw, ph = 33, 17, 50, 21
    case = make_case(w, h, pw, ph, seed=9, cap=6.5)
    r = rt.Renderer(host.Scene.config(1), _cam(*HAND_CUR, w=w, h=h))
    other = rt.Context(0)
    try:
        rt.initial_uniforms(_cam(*HAND_OLD, w=pw, h=ph), r.shader.program)
        view = r.shader.view()
        rt.initial_uniforms(_cam(*HAND_CUR, w=w, h=h), r.shader.program)
        rays = r.pick(_all_pixels(w, h), sample=2, return_rays=True)[1].reshape(h, w, 6)
        marks = np.full((h, w, 4), 7.0, F)
        host_arrays = {"g": case["guide"], "s": case["sums"], "pg": case["prev_guide"], "ph": case["prev_hist"], "ho": marks, "mo": marks,
                       "small": marks[:16, :32], "pg2": case["prev_guide"][:20, :49]}
        dev = {k: _wrapped(r.ctx, a) for k, a in host_arrays.items()}
        tex = {k: v[1].h for k, v in dev.items()}
        foreign = _wrapped(other, marks)
        V, O = rt.ERR_INVALID_VALUE, rt.ERR_INVALID_OPERATION
        pv = lambda v: None if v is None else ctypes.byref(v)    # noqa: E731

        def call(c="c", sample=2, g="g", s="s", spp=3, v=view, pg="pg", ph_="ph", cap=6.5, ho="ho", mo="mo", flags=0):
            t = lambda k: k if (k is None or not isinstance(k, str)) else tex[k]   # noqa: E731
            return L.tdt_image_reproject(r.shader.h if c == "c" else c, sample, t(g), t(s), spp, pv(v), t(pg), t(ph_), cap, t(ho), t(mo), flags)

        def degenerate(**kw):
            d = rt.VIEW.from_buffer_copy(view)
            for k, val in kw.items():
                setattr(d, k, val)
            return d
        V3 = ctypes.c_float * 3
        rows = [
            (V, dict(c=None)), (V, dict(g=None)), (V, dict(s=None)), (V, dict(ho=None)),
            (V, dict(v=None)), (V, dict(pg=None)), (V, dict(ph_=None)), (V, dict(v=None, pg=None)), (V, dict(pg=None, ph_=None)),
            (V, dict(sample=-1)), (V, dict(spp=0)), (V, dict(spp=-3)), (V, dict(flags=1)),
            (V, dict(cap=0.5)), (V, dict(cap=float("nan"))), (V, dict(cap=-2.0)),
            (V, dict(g="small")), (V, dict(s="small")), (V, dict(ho="small")), (V, dict(mo="small")),
            (V, dict(pg="pg2")),
            (V, dict(v=degenerate(image_width=1))), (V, dict(v=degenerate(image_height=1))), (V, dict(v=degenerate(image_width=0))),
            (V, dict(v=degenerate(horizontal=V3(0, 0, 0)))), (V, dict(v=degenerate(vertical=V3(*view.horizontal)))),
            (V, dict(v=degenerate(origin=V3(float("inf"), 0, 0)))), (V, dict(v=degenerate(horizontal=V3(float("nan"), 0, 0)))),
            (V, dict(s="g")), (V, dict(ho="s")), (V, dict(ho="g")), (V, dict(mo="g")), (V, dict(mo="ho")), (V, dict(pg="g", ph_="s")),
            (V, dict(ph_="pg")), (V, dict(mo="ph")), (V, dict(ho="pg")),
            (O, dict(c=rt.ComputeShader(r.ctx, rt.PROGRAM_OCTREE_UPDATE).h)),
            (O, dict(g=foreign[1].h)), (O, dict(mo=foreign[1].h)), (O, dict(ph_=foreign[1].h)),
        ]
        for code, kw in rows:
            assert call(**kw) == code, kw
        for part in ((0, 2), (1, 2)):
            r.shader.set_partition(*part)
            assert call() == O, part
        r.shader.set_partition(0, 1)
        assert L.tdt_compute_view(None, pv(view)) == V and L.tdt_compute_view(r.shader.h, None) == V
        assert L.tdt_compute_view(rt.ComputeShader(r.ctx, rt.PROGRAM_OCTREE_UPDATE).h, pv(view)) == O
        assert L.tdt_debug_reproject_counts(None, None) == V and L.tdt_image_clear(None) == V
        r.ctx.finish()
        for k, a in host_arrays.items():
            assert _bits(dev[k][0].cpu().numpy()).tobytes() == _bits(a).tobytes(), k
        assert _bits(foreign[0].cpu().numpy()).tobytes() == marks.tobytes()
        # the call reads no scene buffer: with slots 0, 1, 6, 7 unbound it is the model's bytes (and mean_out may be the sums)
        for slot in (0, 1, 6, 7):
            L.tdt_bind_buffer_base(r.ctx.h, rt.SHADER_STORAGE_BUFFER, slot, None)
        assert call(mo="s") == rt.OK
        counts = r.ctx.reproject_counts()
        m_hist, m_mean, _, _, m_counts = model.reproject(rays, case["guide"], case["sums"], 3, model.view_from_ctypes(view), case["prev_guide"],
                                                         case["prev_hist"], 6.5)
        _same(dev["ho"][0].cpu().numpy(), m_hist, "history")
        _same(dev["s"][0].cpu().numpy(), m_mean, "mean in place")
        assert counts == m_counts and m_counts[1] > 0
        dev["small"][1].clear()
        r.ctx.finish()
        assert not dev["small"][0].cpu().numpy().any()
    finally:
        other.close()
        r.close()


# ---- 7. the demo binary ----------------------------------------------------------------------------------------------------
def test_demo_temporal_turns_by_degrees_and_writes_the_frame(tmp_path):
    """tdt_demo --temporal 8 --denoise 2 --turn 1.5 writes the frame Renderer.render_temporal gives for main.rs's camera yawed 1.5
    DEGREES per frame: the controller's turn_yaw takes units of 2 * turn_rate radians, and the demo converts with its turn_rate."""
    import re
    import subprocess
    from tdt4230_project_raytracing_amd import build
    exe = build.build_demo()
    out = str(tmp_path / "frame.pfm")
    run = subprocess.run([exe, "--config", "1", "--size", f"{W}x{H}", "--temporal", "8", "--denoise", "2", "--turn", "1.5", "--out", out],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    with open(out, "rb") as fh:
        assert fh.readline().strip() == b"PF4" and fh.readline().split() == [str(W).encode(), str(H).encode()]
        fh.readline()
        frame = np.frombuffer(fh.read(), "<f4").reshape(H, W, 4)
    rate = F(0.05)                                                     # demo_main.cpp's with_turn_rate
    c = host.Camera(90.0, W, aspect_ratio=F(W) / F(H), origin=[0.0, -0.1, -0.3], viewport_height=2.0, samples_per_pixel=SPP, max_bounce=6,
                    turn_rate=float(rate))
    units = F(1.5) * F(0.017453292519943295) / (F(2) * rate)
    assert abs(2.0 * float(units) * float(rate) - np.radians(1.5)) < 1e-6          # 1.5 degrees in turn_yaw's units
    first = c.uniforms()
    r = rt.Renderer(host.Scene.config(1), first)
    try:
        for k in range(8):
            if k:
                c.turn_yaw(float(units))
            want = r.render_temporal(cam=c.uniforms(), denoise=2)
        counts = r.ctx.reproject_counts()
    finally:
        r.close()
    # the whole turn is 7 * 1.5 degrees: the angle between the first and the last view's `horizontal`
    h0, h1 = np.array(list(first.horizontal), np.float64), np.array(list(c.uniforms().horizontal), np.float64)
    turned = np.degrees(np.arccos(np.dot(h0, h1) / (np.linalg.norm(h0) * np.linalg.norm(h1))))
    assert abs(turned - 10.5) < 1e-3, turned
    _same(frame, want, "the demo's last frame")
    m = re.search(r"temporal frames 8 keyed (\d+) found (\d+) rejected-key (\d+) rejected-screen (\d+)", run.stdout)
    assert m and tuple(int(v) for v in m.groups()) == counts, run.stdout
    assert counts[1] > 0
