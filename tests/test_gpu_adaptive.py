"""The sampling controller on the GPU (csrc/tdt_adaptive.hip): tdt_image_adapt, its counts and tdt_image_adapt_mean give the bytes
of the numpy model (tests/adaptive_model.py) on hand-made data of every size class, with and without a guide; errors write nothing;
Renderer.render_adaptive — masked trace passes steered by those states — leaves the state, the sums and the resolved frame of
the model's loop over the oracle, bit for bit, with and without the filter; and tdt_demo --adaptive writes render_adaptive's frame."""
import re
import subprocess

import numpy as np
import pytest

import adaptive_model as model
import denoise_model
import variance_model
from image_util import INSIDE_TURNED, _bits, _raises, _wrapped
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

F = np.float32
OUTSIDE = ((0.0, 0.2, 0.9), 0.0, -8.0, 90.0)         # tests/test_gpu_prepass.py's "in front, looking in"
FRAMES = {"config1 inside": (1, INSIDE_TURNED), "config2 outside": (2, OUTSIDE)}
W, H, BATCH, CAP, TOL = 64, 48, 2, 8, 0.05


def _cam(origin, yaw, pitch, fov, w=W, h=H, spp=CAP, bounce=6):
    c = host.Camera(fov, w, aspect_ratio=F(w) / F(h), origin=origin, viewport_height=2.0, samples_per_pixel=spp, max_bounce=bounce)
    if yaw:
        c.turn_yaw(yaw)
    if pitch:
        c.turn_pitch(pitch)
    return c.uniforms()


def _same(got, want, what, exact=None):
    """Bit for bit, but that a computed NaN equals any NaN (the header leaves its sign and payload open); `exact`: the pixels,
    copied ones, where even a NaN must keep its bits."""
    differ = _bits(got) != _bits(want)
    loose = differ & ~(np.isnan(got) & np.isnan(want))
    diff = (loose if exact is None else np.where(exact[..., None], differ, loose)).any(-1)
    at = np.argwhere(diff)[:4]
    assert not diff.any(), (what, int(diff.sum()), at.tolist(), [(got[tuple(p)].tolist(), want[tuple(p)].tolist()) for p in at])


@pytest.fixture(scope="module")
def ctx():
    r = rt.Renderer(host.Scene.config(1), _cam(*INSIDE_TURNED))
    yield r.ctx
    r.close()


def run_adapt(ctx, sums, guide, state, k, limits):
    """tdt_image_adapt and tdt_image_adapt_mean over host arrays: (state_out, counts, means), the inputs checked unchanged."""
    ins = [(a, _wrapped(ctx, a)) for a in (sums, state) + ((guide,) if guide is not None else ())]
    out = _wrapped(ctx, np.full(state.shape, 7.0, F))
    ins[0][1][1].adapt(ins[2][1][1] if guide is not None else None, ins[1][1][1], out[1], k, *limits)
    counts = ctx.adapt_counts()
    img = _wrapped(ctx, sums)
    img[1].adapt_mean(out[1])
    ctx.finish()
    for a, (t, _) in ins:
        assert _bits(t.cpu().numpy()).tobytes() == _bits(a).tobytes()
    return out[0].cpu().numpy(), counts, img[0].cpu().numpy()


# ---- 1. hand-made data -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_guide", [True, False], ids=["guide", "no guide"])
@pytest.mark.parametrize("w,h", model.SIZES, ids=lambda v: str(v))
def test_hand_made_data_is_the_model_bit_for_bit(ctx, w, h, with_guide):
    seen = np.zeros(4, np.int64)
    for n, lim in enumerate(model.LIMITS):
        sums, guide, state = model.make_case(w, h, 7 * n + w)
        guide = guide if with_guide else None
        want, want_counts = model.adapt(sums, guide, state, BATCH, *lim)
        got, counts, means = run_adapt(ctx, sums, guide, state, BATCH, lim)
        _same(got, want, ("state", lim), exact=~model.live(state))
        assert counts == want_counts, lim
        _same(means, model.adapt_mean(sums, want), ("means", lim), exact=want[..., 3] == 0)
        seen += want_counts
    print(f"{w}x{h}: live before, by tolerance, by cap, still live over the limits = {seen.tolist()}")
    if w * h >= 64:
        assert (seen > 0).all()                                          # every outcome is reached


def test_a_pixel_waits_for_the_tile_next_door(ctx):
    """Keys that differ across the 32x8 tile borders, and one noisy pixel on each side of a border: the quiet pixels next to it wait
    when they share its face — through the staged halo — and stop when they do not."""
    w, h = 70, 20
    quiet = (model.lum(np.array([2, 2, 2], F)), 1.0, 1.0, 2.0)
    sums = np.zeros((h, w, 4), F)
    sums[..., :3] = 4.0
    state = np.tile(np.array(quiet, F), (h, w, 1))
    guide = np.zeros((h, w), denoise_model.GUIDE_DTYPE)
    guide["kind"] = 1
    guide["material"] = (np.arange(w)[None, :] >= 40) * 1 + (np.arange(h)[:, None] >= 12) * 2      # faces that end off the tile borders
    for x, y in ((31, 3), (32, 8), (63, 7), (40, 12)):
        sums[y, x, :3] = 8.0                                             # noisy
    lim = (0.01, 0.0, 0, 64)
    want, want_counts = model.adapt(sums, guide, state, BATCH, *lim)
    got, counts, _ = run_adapt(ctx, sums, guide, state, BATCH, lim)
    _same(got, want, "state")
    assert counts == want_counts
    live = got[..., 3] > 0
    assert live[3, 32] and live[7, 31] and live[8, 31] and live[9, 33]    # across the vertical and the horizontal border
    assert live[6, 62] and live[8, 63] and not live[12, 39] and not live[11, 40] and live[13, 41]
    assert int(live.sum()) == 9 + 9 + 9 + 4


def test_errors_write_nothing(ctx):
    sums, guide, state = model.make_case(33, 17, 1)
    t = {k: _wrapped(ctx, a) for k, a in (("sums", sums), ("guide", guide), ("state", state), ("out", np.full(state.shape, 7.0, F)),
                                           ("small", np.zeros((16, 33, 4), F)))}
    tex = {k: v[1] for k, v in t.items()}
    VAL = rt.ERR_INVALID_VALUE
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["state"], tex["out"], 0, 0.05)
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["state"], tex["out"], 2, float("nan"))
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["state"], tex["out"], 2, -0.1)
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["state"], tex["out"], 2, 0.05, float("inf"))
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["state"], tex["out"], 2, 0.05, 0.0, -1)
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["state"], tex["out"], 2, 0.05, 0.0, 0, 0)
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["state"], tex["state"], 2, 0.05)             # in place
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["state"], tex["sums"], 2, 0.05)
    _raises(VAL, tex["sums"].adapt, tex["guide"], tex["small"], tex["out"], 2, 0.05)
    _raises(VAL, tex["sums"].adapt_mean, tex["sums"])
    _raises(VAL, tex["sums"].adapt_mean, tex["small"])
    other = rt.Renderer(host.Scene.config(1), _cam(*INSIDE_TURNED))
    multi = rt.Renderer(host.Scene.config(1), _cam(*INSIDE_TURNED), devices=[0, 0])
    try:
        foreign = rt.Texture.new_2d(other.ctx, 33, 17, bind=False)
        _raises(rt.ERR_INVALID_OPERATION, tex["sums"].adapt, tex["guide"], tex["state"], foreign, 2, 0.05)
        _raises(rt.ERR_INVALID_OPERATION, tex["sums"].adapt_mean, foreign)
        a, b, c = (rt.Texture.new_2d(multi.ctx, 33, 17, bind=False) for _ in range(3))
        _raises(rt.ERR_INVALID_OPERATION, a.adapt, None, b, c, 2, 0.05)
        _raises(rt.ERR_INVALID_OPERATION, a.adapt_mean, b)
        _raises(rt.ERR_INVALID_OPERATION, multi.ctx.adapt_counts)
    finally:
        other.close()
        multi.close()
    ctx.finish()
    for k, a in (("sums", sums), ("state", state), ("out", np.full(state.shape, 7.0, F))):
        assert _bits(t[k][0].cpu().numpy()).tobytes() == _bits(a).tobytes(), k


# ---- 2. the frame ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(oracle):
    """Per frame: the renderer, its guide of sample 0 as the GPU wrote it, and the model's loop over the oracle with that guide."""
    made = {}

    def get(name):
        if name not in made:
            cfg, pose = FRAMES[name]
            scene, cam = host.Scene.config(cfg), _cam(*pose)
            r = rt.Renderer(scene, cam)
            guide_tex = rt.Texture.new_2d(r.ctx, W, H, bind=False)
            r.shader.dispatch_guide(guide_tex)
            guide = guide_tex.read_guide()
            f = model.render_adaptive(oracle, scene, cam, TOL, batch=BATCH, min_samples=4, max_samples=CAP, floor=r.adaptive_floor, guide=guide)
            hist = {int(n): int((f["samples"] == n).sum()) for n in np.unique(f["samples"])}
            print(f"{name}: rounds {f['rounds']}, counts per round {f['counts']}, samples {hist}")
            assert len(hist) > 1 and f["rounds"] == CAP // BATCH          # the masks shrink, and something runs to the cap
            made[name] = dict(r=r, scene=scene, cam=cam, guide=guide, model=f)
        return made[name]
    yield get
    for c in made.values():
        c["r"].close()


@pytest.mark.parametrize("name", list(FRAMES))
def test_the_loop_call_by_call_is_the_models(frames, name):
    """render_adaptive's calls made by hand, the sums and the state read after every round."""
    c = frames(name)
    r, f = c["r"], c["model"]
    cur, other, carry = (rt.Texture.new_2d(r.ctx, W, H, bind=False), rt.Texture.new_2d(r.ctx, W, H, bind=False),
                         rt.Texture.new_2d(r.ctx, 4 * W, H, bind=False))
    guide = rt.Texture.new_2d(r.ctx, W, H, bind=False)
    r.texture.clear()
    sums, state = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    for k in range(f["rounds"]):
        r.shader.dispatch_accumulate_masked(W + 1, H + 1, 1, k * BATCH, BATCH, carry.device_ptr(), cur)
        if k == 0:
            r.shader.dispatch_guide(guide)
        r.texture.adapt(guide, cur, other, BATCH, TOL, r.adaptive_floor, 4, CAP)
        cur, other = other, cur
        assert r.ctx.adapt_counts() == f["counts"][k], k
        state, _ = model.adapt(r.texture.read(), c["guide"], state, BATCH, TOL, r.adaptive_floor, 4, CAP)
        _same(cur.read(), state, ("state after round", k))
    _same(r.texture.read(), f["sums"], "sums")
    _same(cur.read(), f["state"], "state")
    assert r.ctx.adapt_counts()[3] == 0


@pytest.mark.parametrize("denoise,sigma", [(0, None), (2, None), (2, rt.VARIANCE_SIGMA)], ids=["raw", "key-only filter", "variance-guided filter"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_render_adaptive_is_the_models_frame(frames, oracle, name, denoise, sigma):
    c = frames(name)
    r, f = c["r"], c["model"]
    r.variance = sigma
    try:
        got = r.render_adaptive(TOL, batch=BATCH, min_samples=4, max_samples=CAP, denoise=denoise)
    finally:
        r.variance = None
    _same(r.adaptive["state"][0].read(), f["state"], "state")
    assert (r.adaptive["samples"]() == f["samples"]).all() and r.adaptive["rounds"] == f["rounds"]
    img = model.adapt_mean(f["sums"], f["state"])
    if denoise and sigma is None:
        img = denoise_model.denoise(img, c["guide"], denoise)
    elif denoise:
        img = variance_model.denoise_variance(img, c["guide"], denoise, sigma)
    resolved = oracle.resolve(c["cam"], img, 1)
    cov = np.zeros((H, W), bool)
    cov[:(H + 1) // 32 * 32, :(W + 1) // 32 * 32] = True                  # what a dispatch of (W + 1, H + 1) covers
    _same(got, np.where(cov[..., None], resolved, img), "frame")
    # and the frame after it is an ordinary one
    _same(r.render()[cov], oracle.render(c["scene"], c["cam"], threads=8)[cov], "a plain frame afterwards")


# ---- 3. the demo -----------------------------------------------------------------------------------------------------------
def test_demo_adaptive_writes_the_frame(tmp_path):
    from tdt4230_project_raytracing_amd import build
    exe = build.build_demo()
    out = str(tmp_path / "frame.pfm")
    run = subprocess.run([exe, "--config", "1", "--size", f"{W}x{H}", "--spp", str(CAP), "--adaptive", str(TOL), "--denoise", "2", "--variance", "4",
                          "--out", out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    with open(out, "rb") as fh:
        assert fh.readline().strip() == b"PF4" and fh.readline().split() == [str(W).encode(), str(H).encode()]
        fh.readline()
        frame = np.frombuffer(fh.read(), "<f4").reshape(H, W, 4)
    c = host.Camera(90.0, W, aspect_ratio=F(W) / F(H), origin=[0.0, -0.1, -0.3], viewport_height=2.0, samples_per_pixel=CAP, max_bounce=6,
                    turn_rate=0.05)
    r = rt.Renderer(host.Scene.config(1), c.uniforms())
    try:
        r.variance = 4.0
        want = r.render_adaptive(TOL, denoise=2)
        rounds = r.adaptive["rounds"]
    finally:
        r.close()
    _same(frame, want, "the demo's frame")
    m = re.search(r"adaptive \S+ batch 2 rounds (\d+) mean spp", run.stdout)
    assert m and int(m.group(1)) == rounds, run.stdout
