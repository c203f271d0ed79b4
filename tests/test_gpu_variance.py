"""Luminance variance and the variance-guided filter on the GPU (csrc/tdt_variance.hip, and the moments form of
csrc/tdt_reproject.hip's call): tdt_image_variance, tdt_image_denoise_variance and tdt_image_reproject_moments give the bytes of
the numpy model (tests/variance_model.py) on every path — LDS tiles for steps 1 and 2, gathers above, both scratch sequences, the
temporal and the spatial estimate —; the moments call's history, mean and counts are tdt_image_reproject's on the same inputs;
Renderer.render / render_temporal with renderer.variance set are the model chain over the GPU's own sums, and with it unset the
calls they always made; errors write nothing."""
import numpy as np
import pytest

import denoise_model
import reproject_model
import variance_model as model
from image_util import INSIDE_TURNED, PASSES, SIZES, _all_pixels, _bits, _raises, _wrapped  # noqa: F401
from test_gpu_denoise import make_case
from test_gpu_reproject import PAIRS, SPP, _cam, _cover, _same, _units, gpu_frame, renderers  # noqa: F401
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
SIGMA = 2.0


def variance_case(w, h, seed):
    """(guide, [(name, img, floor)]): test_gpu_denoise.make_case's guide (key patches, islands, holes) and colours (negatives,
    denormals, infinities of one sign, NaNs of one payload), with alpha drawn as a variance: 0 .. 8, so that sigma^2 * alpha lies
    around the squared luminance differences of the colours and the weight keeps some taps and drops others, and exactly zero in a
    box of a quarter of the image, where lim = 0 and pixels are copied.  Three more runs over the same guide: alpha zero everywhere
    without a floor (nothing is filtered) and with one (everything is), and a NaN centre at pixel (0, 0), which keeps no tap at all."""
    img, guide = make_case(w, h, seed)
    rng = np.random.default_rng(seed + 77)
    img[..., 3] = (8.0 * rng.random((h, w))).astype(F)
    img[: (h + 1) // 2, : (w + 1) // 2, 3] = 0.0
    flat = img.copy()
    flat[..., 3] = 0.0
    nan_centre = img.copy()
    nan_centre[0, 0, :3] = np.nan
    nan_centre[0, 0, 3] = 1.0                                         # ((0, 0) is an island, or the only pixel: lim is its own alpha's)
    return guide, [("drawn", img, 0.0), ("no variance", flat, 0.0), ("floor only", flat, 0.75), ("nan centre", nan_centre, 0.0)]


def assert_case_covers(guide, images, w, h):
    """From the model alone: the case holds pixels with a tap kept by luminance, with a tap rejected by it, pixels copied for
    lim <= 0, and kind-0 pixels (the last except at 1x1)."""
    kept_any = rejected_any = copied_any = False
    neighbours_kept = False
    for _, img, floor in images:
        copied, kept, rejected = model.classify(img, guide, 1, SIGMA, floor)
        kept_any |= bool((kept > 0).any())
        neighbours_kept |= bool((kept > 1).any())
        rejected_any |= bool((rejected > 0).any())
        copied_any |= bool(copied.any())
    assert kept_any and rejected_any and copied_any, (w, h, kept_any, rejected_any, copied_any)
    if w * h >= 25:
        assert neighbours_kept, (w, h)                                # not only centre taps
        _, kept, rejected = model.classify(images[0][1], guide, 1, SIGMA)
        assert ((kept > 1) & (rejected > 0)).any(), (w, h)            # one pixel with both
    assert (guide["kind"] == 0).any() or w * h == 1


# ---- the filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_filter_is_the_model_bit_for_bit(w, h):
    guide, images = variance_case(w, h, seed=w * 1000 + h)
    assert_case_covers(guide, images, w, h)
    ctx = rt.Context(0)
    try:
        g_t, g_tex = _wrapped(ctx, guide)
        for name, img, floor in images:
            for passes in PASSES:
                i_t, i_tex = _wrapped(ctx, img)
                i_tex.denoise_variance(g_tex, passes, SIGMA, floor)
                ctx.finish()
                got = i_t.cpu().numpy()
                want = model.denoise_variance(img, guide, passes, SIGMA, floor)
                diff = _bits(got) != _bits(want)
                print(f"{w}x{h} {name} passes {passes}: {int(diff.sum())} of {diff.size} words differ")
                assert not diff.any(), (w, h, name, passes, np.argwhere(diff)[:4].tolist())
            assert _bits(g_t.cpu().numpy()).tobytes() == guide.tobytes()
        i_t, i_tex = _wrapped(ctx, images[0][1])                      # zero passes: nothing happens
        i_tex.denoise_variance(g_tex, 0, SIGMA)
        ctx.finish()
        assert _bits(i_t.cpu().numpy()).tobytes() == _bits(images[0][1]).tobytes()
    finally:
        ctx.close()


# ---- the variance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_variance_is_the_model_bit_for_bit(w, h):
    guide, images = variance_case(w, h, seed=w * 1000 + h + 5)
    img = images[0][1]
    rng = np.random.default_rng(w * 31 + h)
    min_frames = 4.0
    n = np.array([3.0, np.nextafter(F(4), F(0)), 4.0, np.nextafter(F(4), F(9)), 40.0, 0.0, -0.0, -5.0, np.nan, np.inf], F)
    moments = (rng.standard_normal((h, w, 4)) * 2).astype(F)
    moments[..., 2] = n[(np.arange(w * h).reshape(h, w) + int(rng.integers(0, len(n)))) % len(n)]     # (every count occurs where there is room)
    moments[..., 1] = np.abs(moments[..., 1]) * moments[..., 2]       # mostly e2 > mu^2 ..
    special = rng.random((h, w))
    moments[special < 0.1, 1] = 0.0                                   # .. but also e2 < mu^2: clamped
    moments[(special >= 0.1) & (special < 0.15), 0] = F(np.nan)
    moments[(special >= 0.15) & (special < 0.2), 1] = F(np.inf)
    want_spatial = model.variance(img, guide)
    want_temporal = model.variance(img, guide, moments, min_frames)
    keyed = guide["kind"] != 0
    if w * h >= 25:
        assert (want_spatial[..., 3][keyed] > 0).any() and (_bits(want_spatial[..., 3])[keyed] == 0).any()
        used = keyed & (moments[..., 2] >= F(min_frames))
        assert used.any() and (keyed & ~used).any()
        assert (_bits(want_temporal[..., 3]) != _bits(want_spatial[..., 3])).any()
    ctx = rt.Context(0)
    try:
        g_t, g_tex = _wrapped(ctx, guide)
        m_t, m_tex = _wrapped(ctx, moments)
        for want, mom in ((want_spatial, None), (want_temporal, m_tex)):
            i_t, i_tex = _wrapped(ctx, img)
            i_tex.variance(g_tex, mom, min_frames)
            ctx.finish()
            got = i_t.cpu().numpy()
            _same(got[..., :3], img[..., :3], "rgb comes back unchanged")
            diff = _bits(got[..., 3]) != _bits(want[..., 3])
            print(f"{w}x{h} {'temporal' if mom is not None else 'spatial'}: {int(diff.sum())} of {diff.size} variances differ")
            assert not diff.any(), (w, h, np.argwhere(diff)[:4].tolist())
            assert _bits(g_t.cpu().numpy()).tobytes() == guide.tobytes()
            _same(m_t.cpu().numpy(), moments, "the moments are only read")
    finally:
        ctx.close()


# ---- the moments -----------------------------------------------------------------------------------------------------------
def hand_moments(w, h, mf, seed):
    """A moments image whose frame counts sit around mf, at or below zero, or are NaN."""
    rng = np.random.default_rng(seed)
    mf = F(mf)
    n = np.array([F(1), np.nextafter(mf, F(0)), mf, np.nextafter(mf, F(np.inf)), mf * F(3), F(0), F(-0.0), F(-1), F(np.nan)], F)
    m = np.zeros((h, w, 4), F)
    m[..., 2] = n[rng.integers(0, len(n), (h, w))]
    m[..., 0] = (rng.random((h, w)) * 2).astype(F)
    m[..., 1] = (rng.random((h, w)) * 3).astype(F)
    return m


@pytest.mark.parametrize("pair,size", [("yaw", (64, 48)), ("sideways", (64, 48)), ("forward", (64, 48)), ("identical", (64, 48)),
                                       ("yaw", (33, 17)), ("yaw", (2, 2))])
def test_reproject_moments_is_reproject_and_the_model(renderers, pair, size):  # noqa: F811
    r = renderers("config1")
    a, b = PAIRS["config1"][pair]
    w, h = size
    max_samples = 10.0                                                # mf = 10 / 4 = 2.5 frames
    new = lambda: rt.Texture.new_2d(r.ctx, w, h, bind=False)  # noqa: E731
    old = gpu_frame(r, _cam(*a, w=w, h=h), 0, max_samples=max_samples)
    # the first frame: no history, moments (l, l^2, 1, 0)
    hist_tex, mom_tex, mean_tex = new(), new(), new()
    old["sums_tex"].reproject_moments(r.shader, 0, old["guide_tex"], SPP, None, max_samples, hist_out=hist_tex, moments_out=mom_tex, mean_out=mean_tex)
    counts = r.ctx.reproject_counts()
    want = model.reproject_moments(old["rays"], old["guide"], old["sums"], SPP, None, None, None, None, max_samples)
    _same(mom_tex.read(), want[0], "first frame moments")
    _same(hist_tex.read(), old["hist"], "first frame history is tdt_image_reproject's")
    _same(mean_tex.read(), old["mean"], "first frame mean is tdt_image_reproject's")
    assert counts == old["counts"] == want[5]
    assert (want[0][..., 2] == 1).all()
    # the second frame, over hand-made moments of the first
    prev_moments = hand_moments(w, h, max_samples / SPP, seed=w + 7 * h)
    pm_t, pm_tex = _wrapped(r.ctx, prev_moments)
    cur = gpu_frame(r, _cam(*b, w=w, h=h), SPP, prev=old, max_samples=max_samples)        # tdt_image_reproject on these inputs
    hist_tex, mom_tex, mean_tex = new(), new(), new()
    cur["sums_tex"].reproject_moments(r.shader, SPP, cur["guide_tex"], SPP, (old["view"], old["guide_tex"], old["hist_tex"], pm_tex), max_samples,
                                      hist_out=hist_tex, moments_out=mom_tex, mean_out=mean_tex)
    counts = r.ctx.reproject_counts()
    _same(hist_tex.read(), cur["hist"], "history is tdt_image_reproject's")
    _same(mean_tex.read(), cur["mean"], "mean is tdt_image_reproject's")
    assert counts == cur["counts"]
    want = model.reproject_moments(cur["rays"], cur["guide"], cur["sums"], SPP, reproject_model.view_from_ctypes(old["view"]), old["guide"],
                                   old["hist"], prev_moments, max_samples)
    _same(hist_tex.read(), want[1], "history is the model's")
    assert counts == want[5]
    found, Q = want[4], want[3]
    if size != (2, 2):
        n = prev_moments[Q[..., 1], Q[..., 0], 2][found]
        mf = F(max_samples) / F(SPP)
        assert (n > mf).any() and ((n > 0) & (n <= mf)).any() and (~(n > 0)).any()      # above the cap, below it, and no frames behind
        assert (want[0][..., 2][found] == F(1) + mf).any() and (want[0][..., 2] == 1).any()
    _same(mom_tex.read(), want[0], "moments")
    _same(pm_t.cpu().numpy(), prev_moments, "the earlier moments are only read")
    # the mean written over the sums: the moments still see the sums
    mom2 = new()
    hist2 = new()
    cur["sums_tex"].reproject_moments(r.shader, SPP, cur["guide_tex"], SPP, (old["view"], old["guide_tex"], old["hist_tex"], pm_tex), max_samples,
                                      hist_out=hist2, moments_out=mom2, mean_out=cur["sums_tex"])
    _same(mom2.read(), want[0], "moments with the mean in place")
    _same(cur["sums_tex"].read(), cur["mean"], "mean in place")


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_render_with_variance_is_the_model_chain(oracle):
    scene = host.Scene.config(1)
    cam = _cam(*INSIDE_TURNED)
    cover = _cover(W, H)
    sigma = rt.VARIANCE_SIGMA
    r = rt.Renderer(scene, cam)
    try:
        assert r.variance is None
        plain = r.render(*cover)
        key_only = r.render(*cover, denoise=3)
        # a renderer that never heard of the feature: the calls render(denoise=3) made before it existed
        r.shader.dispatch_accumulate(*cover, 1, 0, SPP)
        sums = r.texture.read()
        guide_tex = rt.Texture.new_2d(r.ctx, W, H, bind=False)
        r.shader.dispatch_guide(guide_tex)
        guide = guide_tex.read_guide()
        r.texture.denoise(guide_tex, 3)
        r.shader.dispatch_resolve(*cover, 1, SPP)
        assert r.texture.read().tobytes() == key_only.tobytes()
        r.variance = sigma
        got = r.render(*cover, denoise=3)
        with_variance = model.variance(sums, guide)
        copied, kept, rejected = model.classify(with_variance, guide, 1, sigma)
        assert (kept > 1).any() and (rejected > 0).any()
        want = oracle.resolve(cam, model.denoise_variance(with_variance, guide, 3, sigma), SPP, dispatch=cover)
        _same(got, want, "render(denoise=3) with renderer.variance")
        assert got.tobytes() != key_only.tobytes() and got.tobytes() != plain.tobytes()
        assert r.render(*cover).tobytes() == plain.tobytes()          # without denoise the setting does nothing
        r.variance = None
        assert r.render(*cover, denoise=3).tobytes() == key_only.tobytes()
    finally:
        r.close()


def test_render_temporal_with_variance_is_the_model_chain(oracle):
    """Three frames under a yaw of 1 degree per frame, the temporal estimate trusted from two frames on, so that the second and
    the third frame mix both estimates."""
    scene = host.Scene.config(1)
    o, yaw, pitch, fov = INSIDE_TURNED
    cams = [_cam(o, yaw + _units(1.0) * k, pitch, fov) for k in range(3)]
    cover = _cover(W, H)
    sigma, max_samples, min_frames = rt.VARIANCE_SIGMA, 64.0, 2.0
    a, b, c = rt.Renderer(scene, cams[0]), rt.Renderer(scene, cams[0]), rt.Renderer(scene, cams[0])
    try:
        a.variance, a.variance_min_frames = sigma, min_frames
        prev, temporal_used = None, 0
        for k, cam in enumerate(cams):
            got = a.render_temporal(*cover, cam=cam if k else None, denoise=2, max_samples=max_samples)
            untouched = c.render_temporal(*cover, cam=cam if k else None, denoise=2, max_samples=max_samples)      # variance None
            f = gpu_frame(b, cam, k * SPP)                             # the GPU's own sums, guide and rays of frame k
            if prev is None:
                mom, hist, mean, _, found, counts = model.reproject_moments(f["rays"], f["guide"], f["sums"], SPP, None, None, None, None, max_samples)
            else:
                mom, hist, mean, _, found, counts = model.reproject_moments(f["rays"], f["guide"], f["sums"], SPP,
                                                                            reproject_model.view_from_ctypes(prev["view"]), prev["guide"], prev["hist"],
                                                                            prev["moments"], max_samples)
            assert a.ctx.reproject_counts() == counts
            keyed = f["guide"]["kind"] != 0
            temporal_used += int((keyed & (mom[..., 2] >= F(min_frames))).sum())
            if k:
                assert counts[1] > 0 and (keyed & (mom[..., 2] >= F(min_frames))).any() and (keyed & (mom[..., 2] < F(min_frames))).any()
            img = model.denoise_variance(model.variance(mean, f["guide"], mom, min_frames), f["guide"], 2, sigma)
            _same(got, oracle.resolve(cam, img, 1, dispatch=cover), f"frame {k}")
            # the renderer without the setting runs the calls it always ran
            _same(untouched, oracle.resolve(cam, denoise_model.denoise(mean, f["guide"], 2), 1, dispatch=cover), f"frame {k}, variance None")
            assert got.tobytes() != untouched.tobytes()
            prev = {"view": f["view"], "guide": f["guide"], "hist": hist, "moments": mom}
        assert temporal_used > 0
        assert "moments" not in c.temporal                            # two more textures only when asked for
    finally:
        a.close()
        b.close()
        c.close()


def test_multi_device_context_runs_on_the_first_device():
    """A context over two shares of device 0: both calls work on the assembled frame."""
    scene = host.Scene.config(1)
    cam = _cam(*INSIDE_TURNED)
    r = rt.Renderer(scene, cam, devices=[0, 0])
    try:
        frame = r.render(*_cover(W, H))
        tex = rt.Texture.new_2d(r.ctx, W, H, bind=False)
        r.shader.dispatch_guide(tex)
        guide = tex.read_guide()
        r.texture.variance(tex)
        want = model.variance(frame, guide)
        _same(r.texture.read(), want, "variance")
        assert (want[..., 3] > 0).any()
        r.texture.denoise_variance(tex, 2, 3.0)
        _same(r.texture.read(), model.denoise_variance(want, guide, 2, 3.0), "filter")
    finally:
        r.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(1)
    r = rt.Renderer(scene, _cam(*INSIDE_TURNED, w=33, h=17))
    other = rt.Context(0)
    try:
        guide, images = variance_case(33, 17, 7)
        img = images[0][1]
        arrays = {"img": img, "guide": guide, "moments": hand_moments(33, 17, 2.5, 1), "hist": img * F(2), "mom_out": img * F(3),
                  "prev_guide": guide, "prev_hist": img * F(4), "prev_mom": hand_moments(33, 17, 2.5, 2)}
        held = {k: _wrapped(r.ctx, v) for k, v in arrays.items()}
        tex = {k: v[1] for k, v in held.items()}
        small_t, small = _wrapped(r.ctx, img[:16, :32])               # another size
        far_t, far = _wrapped(other, img)                             # another context
        V, O = rt.ERR_INVALID_VALUE, rt.ERR_INVALID_OPERATION
        i, g, m = tex["img"], tex["guide"], tex["moments"]
        # tdt_image_variance
        assert L.tdt_image_variance(None, g.h, None, 4.0, 0) == V and L.tdt_image_variance(i.h, None, None, 4.0, 0) == V
        assert L.tdt_image_variance(i.h, g.h, None, 4.0, 1) == V
        _raises(V, small.variance, g)
        _raises(V, i.variance, g, small)
        _raises(V, i.variance, i)
        _raises(V, i.variance, g, i)
        _raises(V, i.variance, g, g)
        for bad in (0.5, 0.0, -1.0, float("nan")):
            _raises(V, i.variance, g, m, bad)
        _raises(O, i.variance, far)
        _raises(O, i.variance, g, far)
        # tdt_image_denoise_variance
        assert L.tdt_image_denoise_variance(None, g.h, 1, 1.0, 0.0, 0) == V and L.tdt_image_denoise_variance(i.h, None, 1, 1.0, 0.0, 0) == V
        assert L.tdt_image_denoise_variance(i.h, g.h, 1, 1.0, 0.0, 1) == V
        _raises(V, small.denoise_variance, g, 1, 1.0)
        _raises(V, i.denoise_variance, i, 1, 1.0)
        _raises(V, i.denoise_variance, g, -1, 1.0)
        _raises(V, i.denoise_variance, g, 9, 1.0)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            _raises(V, i.denoise_variance, g, 1, bad)
        for bad in (-0.5, float("inf"), float("nan")):
            _raises(V, i.denoise_variance, g, 1, 1.0, bad)
        _raises(O, i.denoise_variance, far, 1, 1.0)
        # tdt_image_reproject_moments
        view = r.shader.view()
        prev = (view, tex["prev_guide"], tex["prev_hist"], tex["prev_mom"])
        ok = dict(hist_out=tex["hist"], moments_out=tex["mom_out"])
        assert L.tdt_image_reproject_moments(None, 0, g.h, i.h, 4, None, None, None, None, 64.0, tex["hist"].h, tex["mom_out"].h, None, 0) == V
        assert L.tdt_image_reproject_moments(r.shader.h, 0, g.h, i.h, 4, None, None, None, None, 64.0, tex["hist"].h, None, None, 0) == V
        assert L.tdt_image_reproject_moments(r.shader.h, 0, g.h, i.h, 4, None, None, None, None, 64.0, tex["hist"].h, tex["mom_out"].h, None, 1) == V
        _raises(V, i.reproject_moments, r.shader, 0, g, 4, (view, tex["prev_guide"], tex["prev_hist"], None), **ok)       # prev_* come together
        _raises(V, i.reproject_moments, r.shader, 0, g, 4, (None, None, None, tex["prev_mom"]), **ok)
        _raises(V, i.reproject_moments, r.shader, 0, g, 4, (view, tex["prev_guide"], tex["prev_hist"], small), **ok)      # sizes
        _raises(V, i.reproject_moments, r.shader, 0, g, 4, prev, hist_out=tex["hist"], moments_out=small)
        _raises(V, i.reproject_moments, r.shader, 0, g, 4, prev, hist_out=tex["hist"], moments_out=tex["hist"])           # shared memory
        _raises(V, i.reproject_moments, r.shader, 0, g, 4, prev, hist_out=tex["hist"], moments_out=tex["prev_mom"])
        _raises(V, i.reproject_moments, r.shader, 0, g, 4, prev, mean_out=tex["mom_out"], **ok)
        _raises(V, i.reproject_moments, r.shader, 0, g, 0, prev, **ok)
        _raises(V, i.reproject_moments, r.shader, -1, g, 4, prev, **ok)
        _raises(V, i.reproject_moments, r.shader, 0, g, 4, prev, 0.5, **ok)
        _raises(O, i.reproject_moments, r.shader, 0, g, 4, (view, tex["prev_guide"], tex["prev_hist"], far), **ok)
        _raises(O, i.reproject_moments, r.shader, 0, g, 4, prev, hist_out=tex["hist"], moments_out=far)
        _raises(O, i.reproject_moments, rt.ComputeShader(r.ctx, rt.PROGRAM_OCTREE_UPDATE), 0, g, 4, prev, **ok)
        for part in ((0, 2), (1, 2)):
            r.shader.set_partition(*part)
            _raises(O, i.reproject_moments, r.shader, 0, g, 4, prev, **ok)
        r.shader.set_partition(0, 1)
        r.ctx.finish()
        other.finish()
        for k, (t, _) in held.items():
            assert _bits(t.cpu().numpy()).tobytes() == _bits(arrays[k]).tobytes(), k
        assert _bits(far_t.cpu().numpy()).tobytes() == _bits(img).tobytes() and _bits(small_t.cpu().numpy()).tobytes() == _bits(img[:16, :32]).tobytes()
        i.reproject_moments(r.shader, 0, g, 4, prev, mean_out=i, **ok)                     # and the whole call is accepted: mean_out == sums
        r.ctx.finish()
    finally:
        other.close()
        r.close()
