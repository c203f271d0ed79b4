"""Guide-keyed upsampling on the GPU (csrc/tdt_upsample.hip): the image and the counts are the bytes of the numpy model
(tests/upsample_model.py) on hand-made data and on real frames traced at two resolutions; Renderer.render_upsampled is the chain
accumulate, two guides, upsample, (filter,) resolve call by call and leaves the renderer as it found it; errors write nothing; a
multi-device context gives the single-device bytes; tdt_demo --upsample writes render_upsampled's frame; and on the edge pixels of a
real frame the keyed call is closer to the converged picture than plain bilinear magnification."""
import re
import subprocess

import numpy as np
import pytest

import upsample_model as model
from image_util import INSIDE_TURNED, _bits, _wrapped
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

F = np.float32
SPP = 4
CLOSE_UP = ((-0.2503, -0.2497, -0.45), 0.0, 0.0, 3.0)                 # tests/test_gpu_reproject.py's: a demo voxel is twenty pixels wide
POSES = {"config1": INSIDE_TURNED, "demo": CLOSE_UP}


def _cam(origin, yaw, pitch, fov, w, h, spp=SPP, bounce=6):
    c = host.Camera(fov, w, aspect_ratio=np.float32(w) / np.float32(h), origin=origin, viewport_height=2.0, samples_per_pixel=spp,
                    max_bounce=bounce)
    if yaw:
        c.turn_yaw(yaw)
    if pitch:
        c.turn_pitch(pitch)
    return c.uniforms()


def _cover(w, h):
    """A dispatch whose 32x32 work-groups cover all of w x h."""
    return -(-w // 32) * 32, -(-h // 32) * 32


def _same(got, want, what):
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _scene(name):
    return host.Scene.demo() if name == "demo" else host.Scene.config(1)


@pytest.fixture(scope="module")
def renderers():
    made = {}

    def get(name):
        if name not in made:
            made[name] = rt.Renderer(_scene(name), _cam(*POSES[name], 64, 48))
        return made[name]
    yield get
    for r in made.values():
        r.close()


def run_case(ctx, case):
    """tdt_image_upsample over the arrays of a hand-made case, dst pre-filled with marks: (image, counts), the inputs checked unchanged."""
    dst_guide, src, src_guide = case
    H, W = dst_guide.shape
    ins = [_wrapped(ctx, a) for a in (dst_guide, src, src_guide)]
    out = _wrapped(ctx, np.full((H, W, 4), 7.0, F))
    out[1].upsample(ins[0][1], ins[1][1], ins[2][1])
    counts = ctx.upsample_counts()
    for (t, _), a, k in zip(ins, case, ("dst_guide", "src", "src_guide")):
        assert _bits(t.cpu().numpy()).tobytes() == _bits(a).tobytes(), k
    return out[0].cpu().numpy(), counts


# ---- 1. hand-made data -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,w,h,seed", model.HAND_CASES, ids=lambda v: str(v))
def test_hand_made_data_is_the_model_bit_for_bit(renderers, W, H, w, h, seed):
    case = model.make_case(W, H, w, h, seed)
    want, cls = model.upsample(*case)
    got, counts = run_case(renderers("config1").ctx, case)
    print(f"{W}x{H} <- {w}x{h}: pixels, bilinear, ring, holes = {model.histogram(cls)} (GPU {counts})")
    _same(got, want, "image")
    assert counts == model.histogram(cls)


# ---- 2. real frames --------------------------------------------------------------------------------------------------------
def gpu_frames(r, pose, W, H, w, h, spp=SPP):
    """On r's context: the sums of `spp` samples and the guide under pose's camera at W x H with image_width / image_height set to
    w x h (the same frustum), the guide at W x H, and tdt_image_upsample over them."""
    cam = _cam(*pose, W, H, spp=spp)
    rt.initial_uniforms(cam, r.shader.program)
    r.shader.program.set_i32("camera.image_width", w)
    r.shader.program.set_i32("camera.image_height", h)
    f = {"low_tex": rt.Texture.new_2d(r.ctx, w, h)}                   # (bound)
    r.shader.dispatch_accumulate(*_cover(w, h), 1, 0, spp)
    f["low_guide_tex"] = rt.Texture.new_2d(r.ctx, w, h, bind=False)
    r.shader.dispatch_guide(f["low_guide_tex"])
    r.shader.program.set_i32("camera.image_width", W)               # (host.Camera derives its height from the aspect ratio: 66 x 50 gives 49)
    r.shader.program.set_i32("camera.image_height", H)
    f["guide_tex"] = rt.Texture.new_2d(r.ctx, W, H, bind=False)
    r.shader.dispatch_guide(f["guide_tex"])
    f["out_tex"] = rt.Texture.new_2d(r.ctx, W, H, bind=False)
    f["out_tex"].upsample(f["guide_tex"], f["low_tex"], f["low_guide_tex"])
    f["counts"] = r.ctx.upsample_counts()
    f["low"], f["low_guide"], f["guide"], f["out"] = f["low_tex"].read(), f["low_guide_tex"].read_guide(), f["guide_tex"].read_guide(), f["out_tex"].read()
    r.texture.bind()
    return f


@pytest.mark.parametrize("W,H,w,h", [(64, 48, 32, 24), (66, 50, 22, 17)])
@pytest.mark.parametrize("name", ["config1", "demo"])
def test_real_frames_are_the_model_bit_for_bit(renderers, name, W, H, w, h):
    f = gpu_frames(renderers(name), POSES[name], W, H, w, h)
    want, cls = model.upsample(f["guide"], f["low"], f["low_guide"])
    hist = model.histogram(cls)
    print(f"{name} {W}x{H} <- {w}x{h}: pixels, bilinear, ring, holes = {hist} (GPU {f['counts']})")
    assert hist[1] > 0 and len(np.unique(_bits(f["guide"]).reshape(H, W, 4)[..., :3].reshape(-1, 3), axis=0)) > 1    # more than one surface in view
    _same(f["out"], want, "image")
    assert f["counts"] == hist


# ---- 3. the frame ----------------------------------------------------------------------------------------------------------
def chain(b, scale, denoise, cover):
    """render_upsampled's frame call by call on renderer b, the upsampled sums checked against the model on the way."""
    W, H, spp = b.camera.image_width, b.camera.image_height, b.camera.samples_per_pixel
    lw, lh = -(-W // scale), -(-H // scale)
    low, low_guide, guide = rt.Texture.new_2d(b.ctx, lw, lh), rt.Texture.new_2d(b.ctx, lw, lh, bind=False), rt.Texture.new_2d(b.ctx, W, H, bind=False)
    b.shader.program.set_i32("camera.image_width", lw)
    b.shader.program.set_i32("camera.image_height", lh)
    b.shader.dispatch_accumulate(*_cover(lw, lh), 1, 0, spp)
    b.shader.dispatch_guide(low_guide)
    b.shader.program.set_i32("camera.image_width", W)
    b.shader.program.set_i32("camera.image_height", H)
    b.texture.bind()
    b.shader.dispatch_guide(guide)
    b.texture.upsample(guide, low, low_guide)
    want, cls = model.upsample(guide.read_guide(), low.read(), low_guide.read_guide())
    _same(b.texture.read(), want, "upsampled sums")
    if denoise > 0:
        if b.variance is None:
            b.texture.denoise(guide, denoise)
        else:
            b.texture.variance(guide)
            b.texture.denoise_variance(guide, denoise, b.variance)
    b.shader.dispatch_resolve(*cover, 1, spp)
    return b.texture.read(), model.histogram(cls)


@pytest.mark.parametrize("W,H,scale,denoise,variance", [(64, 48, 2, 0, None), (64, 48, 2, 2, None), (64, 48, 2, 0, 4.0), (64, 48, 2, 2, 4.0),
                                                        (66, 50, 3, 1, None)])
def test_render_upsampled_is_the_chain(W, H, scale, denoise, variance):
    scene, cam = host.Scene.config(1), _cam(*INSIDE_TURNED, W, H)
    W, H = cam.image_width, cam.image_height                          # (host.Camera derives the height from the aspect ratio: 66 x 50 gives 49)
    cover = _cover(W, H)
    a, b = rt.Renderer(scene, cam), rt.Renderer(scene, cam)
    try:
        a.variance = b.variance = variance
        plain = a.render(*cover)
        got = a.render_upsampled(scale, denoise, *cover)
        want, hist = chain(b, scale, denoise, cover)
        _same(got, want, "frame")
        assert a.ctx.upsample_counts() == hist
        assert (a.low[0].width(), a.low[0].height()) == (-(-W // scale), -(-H // scale))
        assert got.tobytes() != plain.tobytes()
        v = a.shader.view()
        assert (v.image_width, v.image_height) == (W, H)
        _same(a.render_upsampled(scale, denoise, *cover), want, "a second frame")
        a.variance = None
        assert a.render(*cover).tobytes() == plain.tobytes()          # the default path is what it was
        # a frame that raises half-way (no cells bound: the low accumulate is refused) leaves the full uniforms and binding too
        rt.lib().tdt_bind_buffer_base(a.ctx.h, rt.SHADER_STORAGE_BUFFER, 0, None)
        with pytest.raises(rt.TdtError):
            a.render_upsampled(scale, denoise, *cover)
        a.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, a.vbos[0])
        v = a.shader.view()
        assert (v.image_width, v.image_height) == (W, H)
        assert a.render(*cover).tobytes() == plain.tobytes()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("denoise", [0, 2])
def test_scale_one_goes_through_the_call_and_is_render(denoise):
    """With equal sizes and equal guides the call is the identity wherever the sums hold no -0 (the model says where): on this
    frame everywhere, so render_upsampled(1, N) is render(denoise=N) byte for byte — and the call ran, as its counts show."""
    W, H = 64, 48
    scene, cam, cover = host.Scene.config(1), _cam(*INSIDE_TURNED, W, H), _cover(W, H)
    a = rt.Renderer(scene, cam)
    try:
        a.shader.dispatch_accumulate(*cover, 1, 0, SPP)
        sums = a.texture.read()
        guide = rt.Texture.new_2d(a.ctx, W, H, bind=False)
        a.shader.dispatch_guide(guide)
        g = guide.read_guide()
        ident, cls = model.upsample(g, sums, g)
        assert (cls == 1).all()
        assert _bits(ident).tobytes() == _bits(sums).tobytes()        # (a fact about this frame's sums: no -0, no NaN)
        want = a.render(*cover, denoise=denoise) if denoise else a.render(*cover)
        assert a.ctx.upsample_counts() == (0, 0, 0, 0)
        got = a.render_upsampled(1, denoise, *cover)
        assert a.ctx.upsample_counts() == (W * H, W * H, 0, 0)
        _same(got, want, "frame")
    finally:
        a.close()


def test_render_upsampled_refuses_what_it_cannot_do():
    scene = host.Scene.config(1)
    cam = _cam(*INSIDE_TURNED, 64, 48)
    multi, tiles = rt.Renderer(scene, cam, devices=[0, 0]), rt.Renderer(scene, cam, tile_buffer_tiles=2)
    try:
        for r in (multi, tiles):
            with pytest.raises(ValueError):
                r.render_upsampled(2)
        for bad in (0, -2, 2.0, "2"):
            with pytest.raises(ValueError):
                tiles.render_upsampled(bad)
    finally:
        multi.close()
        tiles.close()


# ---- 4. errors, several devices --------------------------------------------------------------------------------------------
def test_errors_write_nothing_and_leave_the_counts():
    L = rt.lib()
    W, H, w, h, seed = model.MULTI_CASE
    dst_guide, src, src_guide = model.make_case(W, H, w, h, seed)
    ctx, other = rt.Context(0), rt.Context(0)
    try:
        marks = np.full((H, W, 4), 7.0, F)
        long_row = np.full((1, 32769, 4), 7.0, F)
        host_arrays = {"d": marks, "dg": dst_guide, "s": src, "sg": src_guide, "d_small": marks[:H - 1], "dg_small": _bits(dst_guide).reshape(H, W, 4)[:, :W - 1],
                       "s_small": src[:, :w - 1], "sg_small": _bits(src_guide).reshape(h, w, 4)[:h - 1], "same1": marks, "same2": marks, "same3": marks,
                       "long_d": long_row, "long_dg": long_row, "tall_d": long_row.reshape(32769, 1, 4), "tall_dg": long_row.reshape(32769, 1, 4),
                       "one": marks[:1, :1], "one_g": marks[:1, :1], "wide_s": np.zeros((h, W + 1, 4), F), "wide_sg": np.zeros((h, W + 1, 4), F),
                       "tall_s": np.zeros((H + 1, w, 4), F), "tall_sg": np.zeros((H + 1, w, 4), F)}
        dev = {k: _wrapped(ctx, a) for k, a in host_arrays.items()}
        tex = {k: v[1].h for k, v in dev.items()}
        # an image that shares memory with dst without being it: dst's rows 1.. as an image one row shorter
        overlap = rt.Texture.wrap_device(ctx, dev["d"][0].data_ptr() + W * 16, W, H - 1, bind=False)
        foreign = _wrapped(other, marks)
        dev["d"][1].upsample(dev["dg"][1], dev["s"][1], dev["sg"][1])
        want, cls = model.upsample(dst_guide, src, src_guide)
        counts = ctx.upsample_counts()
        assert counts == model.histogram(cls)
        host_arrays["d"] = want
        _same(dev["d"][0].cpu().numpy(), want, "the good call")
        V, O = rt.ERR_INVALID_VALUE, rt.ERR_INVALID_OPERATION

        def call(d="d", dg="dg", s="s", sg="sg", flags=0):
            t = lambda k: k if (k is None or not isinstance(k, str)) else tex[k]   # noqa: E731
            return L.tdt_image_upsample(t(d), t(dg), t(s), t(sg), flags)
        rows = [
            (V, dict(d=None)), (V, dict(dg=None)), (V, dict(s=None)), (V, dict(sg=None)),
            (V, dict(flags=1)), (V, dict(flags=0x80000000)),
            (V, dict(dg="dg_small")), (V, dict(d="d_small")), (V, dict(sg="sg_small")), (V, dict(s="s_small")),
            (V, dict(s="wide_s", sg="wide_sg")), (V, dict(s="tall_s", sg="tall_sg")),
            (V, dict(d="long_d", dg="long_dg", s="one", sg="one_g")), (V, dict(d="tall_d", dg="tall_dg", s="one", sg="one_g")),
            (V, dict(dg="d")), (V, dict(sg="s")),
            (V, dict(d="same1", dg="same2", s="same1", sg="same3")), (V, dict(d="same1", dg="same2", s="same3", sg="same1")),
            (V, dict(d="same1", dg="same2", s="same2", sg="same3")), (V, dict(d="same1", dg="same2", s="same3", sg="same2")),
            (V, dict(s=overlap.h, sg="d_small")), (V, dict(s="d_small", sg=overlap.h)),
            (O, dict(d=foreign[1].h)), (O, dict(dg=foreign[1].h)), (O, dict(s=foreign[1].h)), (O, dict(sg=foreign[1].h)),
        ]
        for code, kw in rows:
            assert call(**kw) == code, kw
            assert ctx.upsample_counts() == counts, kw
        assert L.tdt_debug_upsample_counts(None, None) == V and L.tdt_debug_upsample_counts(ctx.h, None) == V
        assert other.upsample_counts() == (0, 0, 0, 0)                # (no call ever ran there)
        ctx.finish()
        for k, a in host_arrays.items():
            assert _bits(dev[k][0].cpu().numpy()).tobytes() == _bits(a).tobytes(), k
        assert _bits(foreign[0].cpu().numpy()).tobytes() == marks.tobytes()
    finally:
        other.close()
        ctx.close()


def test_multi_device_context_runs_on_the_first_device(renderers):
    case = model.make_case(*model.MULTI_CASE)
    one = run_case(renderers("config1").ctx, case)
    r = rt.Renderer(host.Scene.config(1), _cam(*INSIDE_TURNED, 64, 48), devices=[0, 0])
    try:
        assert r.ctx.upsample_counts() == (0, 0, 0, 0)
        two = run_case(r.ctx, case)
    finally:
        r.close()
    assert one[1][1] > 0 and one[1][2] > 0 and one[1][3] > 0
    _same(two[0], one[0], "image")
    assert two[1] == one[1]


# ---- 5. the demo binary ----------------------------------------------------------------------------------------------------
def test_demo_upsample_writes_the_frame(tmp_path):
    from tdt4230_project_raytracing_amd import build
    W, H = 64, 48
    exe = build.build_demo()
    out = str(tmp_path / "frame.pfm")
    run = subprocess.run([exe, "--config", "1", "--size", f"{W}x{H}", "--upsample", "2", "--denoise", "2", "--variance", "4", "--out", out],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    with open(out, "rb") as fh:
        assert fh.readline().strip() == b"PF4" and fh.readline().split() == [str(W).encode(), str(H).encode()]
        fh.readline()
        frame = np.frombuffer(fh.read(), "<f4").reshape(H, W, 4)
    c = host.Camera(90.0, W, aspect_ratio=F(W) / F(H), origin=[0.0, -0.1, -0.3], viewport_height=2.0, samples_per_pixel=SPP, max_bounce=6,
                    turn_rate=0.05)
    r = rt.Renderer(host.Scene.config(1), c.uniforms())
    try:
        r.variance = 4.0
        want = r.render_upsampled(2, denoise=2)
        counts = r.ctx.upsample_counts()
    finally:
        r.close()
    _same(frame, want, "the demo's frame")
    m = re.search(r"upsample 2 from 32x24 pixels (\d+) bilinear (\d+) ring (\d+) holes (\d+)", run.stdout)
    assert m and tuple(int(v) for v in m.groups()) == counts, run.stdout
    assert counts[0] == W * H and counts[1] > 0


# ---- 6. it helps where it should -------------------------------------------------------------------------------------------
def test_edge_pixels_are_closer_to_the_converged_frame_than_plain_bilinear(renderers):
    """config 1 from inside, 64x48 from 32x24 at 4 spp, against 256 spp of the full-resolution view, in linear radiance, over the
    pixels where stage 1 skipped a tap of positive weight for its key (the edge pixels): the mean squared error of the call is
    below that of plain bilinear magnification, which is the model run with every key zeroed.  Direction only: the ratio is
    printed (and DESIGN.md records it), `< 1` is what is asserted."""
    W, H, w, h = 64, 48, 32, 24
    r = renderers("config1")
    f = gpu_frames(r, INSIDE_TURNED, W, H, w, h)
    r.shader.dispatch_accumulate(*_cover(W, H), 1, 0, 256)
    ref = r.texture.read()[..., :3].astype(np.float64) / 256.0
    _, cls, edge = model.upsample(f["guide"], f["low"], f["low_guide"], with_skipped=True)
    plain, plain_cls = model.upsample(np.zeros_like(f["guide"]), f["low"], np.zeros_like(f["low_guide"]))
    assert (plain_cls == 1).all()
    assert edge.sum() > 100, int(edge.sum())

    def mse(img):
        return float(np.mean((img[..., :3][edge].astype(np.float64) / SPP - ref[edge]) ** 2))
    e_call, e_plain = mse(f["out"]), mse(plain)
    hist = model.histogram(cls)
    print(f"edge pixels {int(edge.sum())} of {W * H}: MSE keyed {e_call:.6f}, plain bilinear {e_plain:.6f}, ratio {e_call / e_plain:.3f}; "
          f"bilinear / ring / holes = {hist[1:]}, hole share {hist[3] / hist[0]:.4f}")
    assert e_plain > 0
    assert e_call / e_plain < 1
