"""Guide images and the denoiser on the GPU (csrc/tdt_denoise.hip): the guide is pick's first hit, four words of it per texel;
the filter gives the bytes of the numpy model (tests/denoise_model.py) on every path — LDS tiles for steps 1 and 2, gathers above;
accumulate, guide, denoise, resolve is what the model makes of the GPU's own sums; errors write nothing."""
import numpy as np
import pytest

import denoise_model as model
from image_util import INSIDE_TURNED, PASSES, SIZES, _all_pixels, _bits, _raises, _wrapped
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

W, H = 64, 48
OUTSIDE = ((0.0, 0.2, 0.9), 0.0, -8.0, 90.0)         # (origin, yaw, pitch, fov), as tests/test_gpu_raycast.py poses its cameras
INSIDE = ((0.0, -0.1, -0.3), 0.0, 0.0, 90.0)
COVER = (64, 64)                                     # a dispatch whose 32x32 work-groups cover all of 64x48


def _cam(origin, yaw, pitch, fov, w=W, h=H, spp=4, bounce=6):
    c = host.Camera(fov, w, aspect_ratio=np.float32(w) / np.float32(h), origin=origin, viewport_height=2.0, samples_per_pixel=spp,
                    max_bounce=bounce)
    if yaw:
        c.turn_yaw(yaw)
    if pitch:
        c.turn_pitch(pitch)
    return c.uniforms()


def _scene(name):
    if name == "demo":
        return host.Scene.demo()
    if name == "config1":
        return host.Scene.config(1)
    return host.Scene.generate(host.SCENE_TERRAIN, 8, 1 << 20, 100, 0x9A1C4)      # the depth-8 terrain of test_gpu_raycast._scenes


# ---- guide equals pick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["demo", "config1", "terrain8"])
def test_guide_is_pick_in_four_words(name):
    scene = _scene(name)
    materials = np.ascontiguousarray(scene.blobs[1]).reshape(-1).view(np.uint32)
    types = materials.reshape(-1, 3)[:, 0]
    flagged = False
    for pose in (OUTSIDE, INSIDE):
        r = rt.Renderer(scene, _cam(*pose))
        try:
            before = r.render(*COVER)
            for sample in (0, 3):
                for gw, gh in ((W, H), (33, 17), (1, 1)):
                    tex = rt.Texture.new_2d(r.ctx, gw, gh, bind=False)
                    hits = r.pick(_all_pixels(gw, gh), sample=sample).reshape(gh, gw)
                    r.shader.dispatch_guide(tex, sample=sample)
                    got = tex.read_guide()
                    want = model.guide_from_hits(hits, materials, False)
                    assert got.tobytes() == want.tobytes(), (name, pose, sample, gw, gh)
                    if (gw, gh) != (W, H):
                        continue
                    keyed = got["kind"] != 0
                    status = hits["status"]
                    assert (status == rt.RAY_HIT).any() and (status == rt.RAY_MISS).any(), (name, pose, sample)
                    assert keyed.any() and (types[got["material"][keyed]] == 0).all()          # without the flag only Lambertian is keyed
                    if name == "demo":                                # hits on metal or glass pass through
                        assert ((status == rt.RAY_HIT) & (hits["fresh_record"] != 0) & ~keyed).any(), (pose, sample)
                    if not flagged:                                   # once per scene: every material keyed
                        r.shader.dispatch_guide(tex, sample=sample, all_materials=True)
                        got_all = tex.read_guide()
                        assert got_all.tobytes() == model.guide_from_hits(hits, None, True).tobytes()
                        if name == "demo":
                            assert (types[got_all["material"][got_all["kind"] != 0]] != 0).any()
                        flagged = True
            after = r.render(*COVER)                                  # cost history, hand-out order and carry untouched
            assert after.tobytes() == before.tobytes()
        finally:
            r.close()
    assert flagged


# ---- filter equals model (at image_util's SIZES and PASSES) ------------------------------------------------------------------
def make_case(w, h, seed):
    """(img (h, w, 4) float32, guide (h, w) GUIDE_DTYPE): random patches of 3-5 keys — two of them differ from the first only by
    one ulp of `plane`, or only in `material` —, single-texel islands with keys of their own, kind-0 holes; colours random with
    negatives, denormals, an infinity and NaN.  One image holds infinities of ONE sign (which one alternates with the seed) and
    NaNs of one payload: inf - inf, and an operation on two different NaNs, produce a NaN whose sign and payload IEEE 754 leaves to
    the implementation, and the contract fixes the operations, not those bits.  Everything else is compared bit for bit."""
    rng = np.random.default_rng(seed)
    base = np.float32(0.3125)
    keys = [(14, 2, base), (14, 2, np.nextafter(base, np.float32(1))), (14, 3, base), (16, 2, base), (5, 7, np.float32(-1.5))]
    keys = keys[: int(rng.integers(3, 6))]
    guide = np.zeros((h, w), model.GUIDE_DTYPE)
    which = np.zeros((h, w), np.int64)
    for _ in range(12):                                               # patches: random boxes painted over each other
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        x1, y1 = x0 + int(rng.integers(1, max(2, w // 2 + 1))), y0 + int(rng.integers(1, max(2, h // 2 + 1)))
        which[y0:y1, x0:x1] = int(rng.integers(0, len(keys)))
    for f, col in (("kind", 0), ("material", 1), ("plane", 2)):
        guide[f] = np.array([k[col] for k in keys])[which]
    guide["t"] = rng.random((h, w), np.float32)
    n = w * h
    flat = guide.reshape(-1)
    spots = rng.permutation(n)
    islands, holes = spots[: max(1, n // 40)], spots[max(1, n // 40): max(1, n // 40) + n // 25]
    for k, p in enumerate(islands):                                   # a key nobody else has
        flat[p] = (20, 100 + k, np.float32(k), 0)
    for p in holes:
        flat[p] = (0, int(rng.integers(0, 4)), 0, 0)
    if n > 1:                                                         # fixed corners: an island, two neighbours of one key, a hole
        flat[0] = (21, 99, 9, 0)
        guide[0, 1 % w] = guide[1 % h, 0]
        flat[n - 1] = (0, 0, 0, 0)
    img = (rng.standard_normal((h, w, 4)) * 3).astype(np.float32)
    special = rng.random((h, w, 4))
    img[special < 0.04] = np.float32(1e-41)                           # denormals
    img[(special >= 0.04) & (special < 0.06)] = np.float32(-3e-42)
    img[(special >= 0.06) & (special < 0.064)] = np.float32(np.inf if seed % 2 else -np.inf)      # (rare: they spread with every pass)
    img[(special >= 0.064) & (special < 0.068)] = np.float32(np.nan)
    return img, guide


@pytest.mark.parametrize("w,h", SIZES)
def test_filter_is_the_model_bit_for_bit(w, h):
    img, guide = make_case(w, h, seed=w * 1000 + h)
    taps = model.kept_taps(guide, 1)
    if w * h > 1:
        assert (taps > 1).any()                                       # (a 1x1 image has the centre tap and nothing else)
    assert (taps == 1).any()
    assert (guide["kind"] == 0).any() or w * h == 1
    ctx = rt.Context(0)
    try:
        g_t, g_tex = _wrapped(ctx, guide)
        for passes in PASSES:
            i_t, i_tex = _wrapped(ctx, img)
            i_tex.denoise(g_tex, passes)
            ctx.finish()
            got = i_t.cpu().numpy()
            want = model.denoise(img, guide, passes)
            diff = _bits(got) != _bits(want)
            print(f"{w}x{h} passes {passes}: {int(diff.sum())} of {diff.size} words differ")
            assert not diff.any(), (w, h, passes, np.argwhere(diff)[:4])
            assert _bits(g_t.cpu().numpy()).tobytes() == guide.tobytes()
        i_t, i_tex = _wrapped(ctx, img)                               # zero passes: nothing happens
        i_tex.denoise(g_tex, 0)
        ctx.finish()
        assert _bits(i_t.cpu().numpy()).tobytes() == _bits(img).tobytes()
    finally:
        ctx.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_accumulate_guide_denoise_resolve(oracle):
    scene = host.Scene.config(1)
    cam = _cam(*INSIDE_TURNED)
    spp = cam.samples_per_pixel
    r = rt.Renderer(scene, cam)
    try:
        plain = r.render(*COVER)
        r.shader.dispatch_accumulate(COVER[0], COVER[1], 1, 0, spp)
        sums = r.texture.read()
        guide_tex = rt.Texture.new_2d(r.ctx, W, H, bind=False)
        r.shader.dispatch_guide(guide_tex)
        guide = guide_tex.read_guide()
        assert (guide["kind"] != 0).any() and (model.kept_taps(guide, 1) > 1).any()
        r.texture.denoise(guide_tex, 3)
        r.shader.dispatch_resolve(COVER[0], COVER[1], 1, spp)
        got = r.texture.read()
        want = oracle.resolve(cam, model.denoise(sums, guide, 3), spp, dispatch=COVER)
        assert got.tobytes() == want.tobytes()
        assert got.tobytes() != plain.tobytes()                      # (it did something)
        assert r.render(*COVER, denoise=3).tobytes() == got.tobytes()
        assert r.render(*COVER).tobytes() == plain.tobytes()         # the default path is what it was
    finally:
        r.close()
    fresh = rt.Renderer(scene, cam)
    try:
        assert fresh.render(*COVER).tobytes() == plain.tobytes()
    finally:
        fresh.close()


def test_multi_device_context_runs_on_the_first_device():
    """A context over two shares of device 0: the guide is the single-device guide, the filter works on the assembled frame."""
    scene = host.Scene.config(1)
    cam = _cam(*INSIDE_TURNED)
    one = rt.Renderer(scene, cam)
    try:
        tex = rt.Texture.new_2d(one.ctx, W, H, bind=False)
        one.shader.dispatch_guide(tex)
        want_guide = tex.read_guide()
    finally:
        one.close()
    r = rt.Renderer(scene, cam, devices=[0, 0])
    try:
        frame = r.render(*COVER)
        tex = rt.Texture.new_2d(r.ctx, W, H, bind=False)
        r.shader.dispatch_guide(tex)
        guide = tex.read_guide()
        assert guide.tobytes() == want_guide.tobytes()
        r.texture.denoise(tex, 2)
        assert r.texture.read().tobytes() == model.denoise(frame, guide, 2).tobytes()
    finally:
        r.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(1)
    r = rt.Renderer(scene, _cam(*INSIDE))
    try:
        img, guide = make_case(33, 17, 7)
        i_t, i_tex = _wrapped(r.ctx, img)
        g_t, g_tex = _wrapped(r.ctx, guide)
        o_t, o_tex = _wrapped(r.ctx, img[:16, :32])                   # another size
        V, O, I = rt.ERR_INVALID_VALUE, rt.ERR_INVALID_OPERATION, rt.ERR_INCOMPLETE
        # NULL handles
        assert L.tdt_image_denoise(None, g_tex.h, 1, 0) == V and L.tdt_image_denoise(i_tex.h, None, 1, 0) == V
        assert L.tdt_dispatch_guide(None, g_tex.h, 0, 0) == V and L.tdt_dispatch_guide(r.shader.h, None, 0, 0) == V
        # the filter's arguments
        _raises(V, o_tex.denoise, g_tex, 1)
        _raises(V, i_tex.denoise, i_tex, 1)
        _raises(V, i_tex.denoise, g_tex, -1)
        _raises(V, i_tex.denoise, g_tex, 9)
        assert L.tdt_image_denoise(i_tex.h, g_tex.h, 1, 1) == V
        # the guide's arguments
        _raises(V, r.shader.dispatch_guide, g_tex, sample=-1)
        assert L.tdt_dispatch_guide(r.shader.h, g_tex.h, 0, 2) == V
        _raises(O, rt.ComputeShader(r.ctx, rt.PROGRAM_OCTREE_UPDATE).dispatch_guide, g_tex)
        for part in ((0, 2), (1, 2)):
            r.shader.set_partition(*part)
            _raises(O, r.shader.dispatch_guide, g_tex)
        r.shader.set_partition(0, 1)
        # missing bindings
        for slot in (0, 6, 7, 1):
            L.tdt_bind_buffer_base(r.ctx.h, rt.SHADER_STORAGE_BUFFER, slot, None)
            _raises(I, r.shader.dispatch_guide, g_tex)
            if slot != 1:
                _raises(I, r.shader.dispatch_guide, g_tex, all_materials=True)
            r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, slot, r.vbos[slot])
        r.ctx.finish()
        assert _bits(i_t.cpu().numpy()).tobytes() == _bits(img).tobytes()
        assert _bits(g_t.cpu().numpy()).tobytes() == guide.tobytes()
        # with slot 1 unbound the all-materials form still runs
        L.tdt_bind_buffer_base(r.ctx.h, rt.SHADER_STORAGE_BUFFER, 1, None)
        r.shader.dispatch_guide(g_tex, all_materials=True)
        assert (g_tex.read_guide()["kind"] != 0).any()
    finally:
        r.close()
