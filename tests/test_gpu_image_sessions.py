"""Image calls and queries queued on ONE long-lived context: the state a context keeps between calls, which the per-unit suites
never reach because each of their cases makes a fresh context or finishes between calls.

- ctx->denoise, the grow-only scratch tdt_image_denoise and tdt_image_denoise_variance both run through: images of seven sizes
  filtered back to back with no finish() and no read between them, so that the second scratch image of a smaller picture sits
  inside a block allocated for a larger one and the block is regrown while earlier passes are still queued.
- ctx->query, the grow-only staging of picks and raycasts: batches that shrink and grow again on one context.
- Renderer.render_temporal's state (frame parity, the moments' sequence, the textures made on first demand) through every
  transition its docstring promises: the moments asked for in mid-sequence, a frame without them, a plain render() in between,
  a reset.

Every comparison is of bits, against the numpy models (denoise_model, variance_model, reproject_model) and the oracle."""
import time

import numpy as np
import pytest

import denoise_model
import reproject_model
import variance_model
from test_gpu_denoise import _wrapped, make_case
from test_gpu_raycast import POSES, _assert_first_hit, _lambertian
from test_gpu_raycast import _cam as _query_cam
from test_gpu_reproject import SPP, _bits, _cam, _cover, _same, _units, gpu_frame
from test_gpu_variance import INSIDE_TURNED, variance_case
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
SIGMA = 2.0

# (call, width, height, passes): the queue of the scratch test
QUEUE = [("denoise", 64, 48, 5),              # allocates 2 * bytes: the three-image opening
         ("denoise_variance", 33, 17, 3),     # the second scratch image at the smaller picture's offset inside the larger block
         ("denoise", 257, 19, 1),             # the copy-back form
         ("denoise_variance", 19, 257, 8),
         ("variance+denoise_variance", 64, 48, 2),      # both on the same image
         ("denoise", 320, 200, 3),            # a regrow while the earlier passes are still queued
         ("denoise", 2, 2, 2)]


@pytest.fixture(scope="module")
def queue_cases():
    """Per entry of QUEUE: (image, guide, the model's result) — computed once, shared by the three runs, never written."""
    out = []
    for k, (call, w, h, passes) in enumerate(QUEUE):
        if call == "denoise":
            img, guide = make_case(w, h, seed=100 + k)
            want = denoise_model.denoise(img, guide, passes)
        else:
            guide, images = variance_case(w, h, seed=100 + k)
            img = images[0][1]
            start = variance_model.variance(img, guide) if call.startswith("variance+") else img
            want = variance_model.denoise_variance(start, guide, passes, SIGMA)
        for a in (img, guide, want):
            a.setflags(write=False)
        out.append((img, guide, want))
    return out


@pytest.mark.parametrize("order,devices", [("forward", None), ("reverse", None), ("first four", [0, 0])])
def test_filters_of_many_sizes_queued_without_a_finish(queue_cases, order, devices):
    """forward: the scratch is allocated for two 64 x 48 images, serves the four smaller pictures that follow and is regrown for the
    320 x 200 one while their passes are still queued; reverse, on a fresh context: the largest image comes first and nothing
    regrows; a two-member context runs the first four entries."""
    entries = {"forward": list(range(7)), "reverse": list(range(6, -1, -1)), "first four": [0, 1, 2, 3]}[order]
    ctx = rt.Context(0, devices=devices)
    t0 = time.perf_counter()
    try:
        held = {k: (_wrapped(ctx, queue_cases[k][0]), _wrapped(ctx, queue_cases[k][1])) for k in entries}      # every input first
        for k in entries:                                             # then the queue: no finish(), no read
            call, w, h, passes = QUEUE[k]
            (_, i_tex), (_, g_tex) = held[k]
            if call == "denoise":
                i_tex.denoise(g_tex, passes)
            else:
                if call.startswith("variance+"):
                    i_tex.variance(g_tex)
                i_tex.denoise_variance(g_tex, passes, SIGMA)
        ctx.finish()
        for k in entries:
            (i_t, _), (g_t, _) = held[k]
            got, want = i_t.cpu().numpy(), queue_cases[k][2]
            diff = _bits(got) != _bits(want)
            print(f"{order} entry {k + 1} {QUEUE[k]}: {int(diff.sum())} of {diff.size} words differ")
            assert not diff.any(), (order, k + 1, QUEUE[k], np.argwhere(diff)[:4].tolist())
            assert _bits(g_t.cpu().numpy()).tobytes() == queue_cases[k][1].tobytes(), (order, k + 1, "the guide is only read")
        print(f"{order}: {time.perf_counter() - t0:.2f} s")
    finally:
        ctx.close()


def test_query_batches_that_shrink_and_grow(oracle):
    """Picks of 1, all 3072, 7 and all 3072 pixels again on one renderer, each followed by a raycast of the rays it returned: the
    staging is sized by the largest batch so far and reused by the smaller ones."""
    scene, alb = _lambertian(host.Scene.config(1))
    cam = _query_cam(*POSES[4])
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.int32)
    rng = np.random.default_rng(11)
    batches = [xy[[1234]], xy, xy[np.sort(rng.choice(len(xy), 7, replace=False))], xy]
    r = rt.Renderer(scene, cam)
    try:
        results = []
        for b in batches:
            hits, rays = r.pick(b, sample=2, return_rays=True)
            again = r.ctx.raycast(rays)
            assert again.tobytes() == hits.tobytes(), len(b)
            results.append((hits, rays))
        full_hits, full_rays = results[1]
        n_hit, n_leaf = _assert_first_hit(oracle, scene, alb, cam, full_hits, full_rays, 2)
        assert n_hit > 0 and n_leaf > 0
        assert _assert_first_hit(oracle, scene, alb, cam, results[3][0], results[3][1], 2) == (n_hit, n_leaf)
        assert results[3][0].tobytes() == full_hits.tobytes() and results[3][1].tobytes() == full_rays.tobytes()
        for b, (hits, rays) in zip(batches, results):                 # the small batches: the full pick's records of those pixels
            at = b[:, 1] * W + b[:, 0]
            assert hits.tobytes() == full_hits[at].tobytes() and rays.tobytes() == full_rays[at].tobytes(), len(b)
    finally:
        r.close()


def test_render_temporal_through_every_transition(oracle):
    """Seven frames under a yaw of 1 degree per frame, max_samples 64, the temporal estimate trusted from two frames on:

        0, 1   variance None, denoise 2     the key-only chain
        2      variance sigma, denoise 2    the moments start here: nothing behind them, frame count 1 everywhere
        3      the same                     moments carried: some pixels take the temporal estimate, some the spatial one
        -      a plain render(denoise=2)    the frame of a fresh renderer; must not disturb what follows
        4      variance sigma, denoise 0    reprojection only: breaks the moments' sequence
        5      variance sigma, denoise 2    the moments restart at count 1 while the history is the whole five frames'
        6      reset, the first camera      frame 0 of a fresh renderer

    Renderer a is under test; b supplies each frame's GPU sums, guide and rays (gpu_frame); the expectation is the model chain."""
    scene = host.Scene.config(1)
    o, yaw, pitch, fov = INSIDE_TURNED
    cams = [_cam(o, yaw + _units(1.0) * k, pitch, fov) for k in range(6)]
    cover = _cover(W, H)
    sigma, max_samples, min_frames = rt.VARIANCE_SIGMA, 64.0, 2.0
    settings = [(None, 2), (None, 2), (sigma, 2), (sigma, 2), (sigma, 0), (sigma, 2)]
    a, b, fresh = rt.Renderer(scene, cams[0]), rt.Renderer(scene, cams[0]), rt.Renderer(scene, cams[0])
    t0 = time.perf_counter()
    try:
        a.variance_min_frames = min_frames
        prev, live, carried = None, False, None                       # carried: the moments had frame 4 not broken their sequence

        def model_frame(f, prev, prev_moments):
            """(moments, history, mean, counts) of a frame with moments behind it (zeros: none)."""
            if prev is None:
                mom, hist, mean, _, _, counts = variance_model.reproject_moments(f["rays"], f["guide"], f["sums"], SPP, None, None, None, None, max_samples)
            else:
                mom, hist, mean, _, _, counts = variance_model.reproject_moments(f["rays"], f["guide"], f["sums"], SPP, reproject_model.view_from_ctypes(prev["view"]),
                                                                                 prev["guide"], prev["hist"], prev_moments, max_samples)
            return mom, hist, mean, counts

        def filtered(mean, guide, mom):
            return variance_model.denoise_variance(variance_model.variance(mean, guide, mom, min_frames), guide, 2, sigma)

        for k, (variance, passes) in enumerate(settings):
            cam = cams[k]
            a.variance = variance
            got = a.render_temporal(*cover, cam=cam if k else None, denoise=passes, max_samples=max_samples)
            f = gpu_frame(b, cam, k * SPP)
            keyed = f["guide"]["kind"] != 0
            zeros = np.zeros((H, W, 4), F)
            with_moments = variance is not None and passes > 0
            mom, hist, mean, counts = model_frame(f, prev, prev["moments"] if prev is not None and live else zeros)
            # the history is tdt_image_reproject's whatever the moments do
            h2, m2, _, _, c2 = reproject_model.reproject(f["rays"], f["guide"], f["sums"], SPP, *((reproject_model.view_from_ctypes(prev["view"]), prev["guide"],
                                                         prev["hist"]) if prev is not None else (None, None, None)), max_samples)
            _same(hist, h2, f"frame {k}: the two models' history")
            _same(mean, m2, f"frame {k}: the two models' mean")
            assert counts == c2
            assert a.ctx.reproject_counts() == counts, k
            if with_moments:
                img = filtered(mean, f["guide"], mom)
            else:
                img = denoise_model.denoise(mean, f["guide"], passes) if passes else mean
            _same(got, oracle.resolve(cam, img, 1, dispatch=cover), f"frame {k}")
            if k == 2:
                assert (mom[..., 2] == 1).all() and counts[1] > 0         # history found, yet no moments behind the frame
            if k == 3:
                assert (keyed & (mom[..., 2] >= F(min_frames))).any() and (keyed & (mom[..., 2] < F(min_frames))).any()
                a.variance = sigma                                    # the plain render in between
                fresh.variance = sigma
                rt.initial_uniforms(cam, fresh.shader.program)
                plain = a.render(*cover, denoise=2)
                assert plain.tobytes() == fresh.render(*cover, denoise=2).tobytes() and plain.tobytes() != got.tobytes()
            if k == 4:                                                # what frame 5 would be given had this frame carried the moments
                carried = model_frame(f, prev, prev["moments"])[0]
                assert live and not with_moments
            if k == 5:
                assert (mom[..., 2] == 1).all() and (hist[..., 3] > F(4 * SPP)).any()     # count 1 everywhere; five frames of history
                alt = filtered(mean, f["guide"], model_frame(f, prev, carried)[0])
                assert (keyed & (model_frame(f, prev, carried)[0][..., 2] >= F(min_frames))).any()
                assert _bits(alt).tobytes() != _bits(img).tobytes(), "the restart of the moments is not observable on this input"
            prev = {"view": f["view"], "guide": f["guide"], "hist": hist, "moments": mom if with_moments else None}
            live = with_moments
        # frame 6: a reset is frame 0 of a fresh renderer with the same settings, and of the model
        a.variance = sigma
        got = a.render_temporal(*cover, cam=cams[0], denoise=2, max_samples=max_samples, reset=True)
        fresh.variance, fresh.variance_min_frames = sigma, min_frames
        want = fresh.render_temporal(*cover, cam=cams[0], denoise=2, max_samples=max_samples)
        assert got.tobytes() == want.tobytes()
        f = gpu_frame(b, cams[0], 0)
        mom, hist, mean, counts = model_frame(f, None, None)
        assert a.ctx.reproject_counts() == counts and counts[1:] == (0, 0, 0)
        _same(got, oracle.resolve(cams[0], filtered(mean, f["guide"], mom), 1, dispatch=cover), "frame 6")
        print(f"render_temporal transitions: {time.perf_counter() - t0:.2f} s")
    finally:
        a.close()
        b.close()
        fresh.close()
