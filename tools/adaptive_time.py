#!/usr/bin/env python3
"""Device-event timing of adaptive sampling (csrc/tdt_rt.hip mask_slots_kernel and the order filter, csrc/tdt_adaptive.hip):

  the masked trace, scene config 2 from outside and config 1 from inside at 1280x720: tdt_dispatch_accumulate_masked of samples
  [4, 6) — mask_slots_kernel, the two filter kernels and the trace — with masks whose live share is 1, 1/2, 1/8 and 1/64 (live
  pixels drawn independently per pixel, the shape noise has), beside the plain tdt_dispatch_accumulate of the same range, whose
  code path this work leaves as it was

  the controller: tdt_image_adapt with and without a guide and tdt_image_adapt_mean beside a device-to-device copy that moves
  their bytes (adapt: 32 B read, 16 B with the guide, and 16 B written per pixel; adapt_mean: 32 B read and 16 B written)

  the frame: Renderer.render_adaptive(0.05, batch 2, cap 64), host synchronisations included, beside the uniform frame at the
  cap (render() with 64 spp), and the mean samples per pixel the adaptive frame spent; the same with batch 8, a quarter of the rounds

    python tools/adaptive_time.py [--reps 15] [--batch 20] [--warmup 3] [--out profiles/adaptive_time_mi355x.txt]

Every time is the median over `reps` windows of `batch` back-to-back calls between two HIP events on the context's stream, divided
by `batch`, after `warmup` untimed windows (traces: batch // 4 calls; whole frames: one).  Prints one JSON line per scene and
writes them to --out.  Measurement only: no test and no bench.py number depends on it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_time import windows  # noqa: E402
from reproject_time import cover  # noqa: E402

W, H, CAP, BATCH, TOL = 1280, 720, 64, 2, 0.05
FRACTIONS = (1, 2, 8, 64)
POSES = {"config2_outside": (2, (0.0, 0.2, 0.9), 0.0, -8.0, 90.0), "config1_inside": (1, (0.1, 0.05, -0.6), 135.0, 10.0, 70.0)}


def time_scene(name, reps, batch, warmup):
    import torch
    from tdt4230_project_raytracing_amd import host, rt
    cfg, origin, yaw, pitch, fov = POSES[name]
    c = host.Camera(fov, W, aspect_ratio=np.float32(W) / np.float32(H), origin=list(origin), viewport_height=2.0, samples_per_pixel=CAP, max_bounce=6)
    if yaw:
        c.turn_yaw(yaw)
    if pitch:
        c.turn_pitch(pitch)
    stream = torch.cuda.Stream(device=0)
    r = rt.Renderer(host.Scene.config(cfg), c.uniforms(), stream=stream.cuda_stream)
    res = {"scene": name, "size": f"{W}x{H}", "reps": reps, "batch": batch}
    try:
        cov, trace = cover(W, H), max(1, batch // 4)
        carry = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda:0")
        mask = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        mask_tex = rt.Texture.wrap_device(r.ctx, mask.data_ptr(), W, H, bind=False)
        torch.cuda.synchronize()
        r.shader.dispatch_accumulate(*cov, 1, 0, 4, carry.data_ptr())       # the state the timed range continues
        res["plain_ms"], res["plain_min_ms"] = windows(stream, lambda: r.shader.dispatch_accumulate(*cov, 1, 4, BATCH, carry.data_ptr()), reps, trace, warmup)
        rng = np.random.default_rng(1)
        for d in FRACTIONS:
            w = np.where(rng.random((H, W)) * d < 1.0, 1.0, -1.0).astype(np.float32)
            r.ctx.finish()
            mask[..., 3].copy_(torch.from_numpy(w))
            torch.cuda.synchronize()
            res[f"masked_1/{d}_ms"], res[f"masked_1/{d}_min_ms"] = windows(
                stream, lambda: r.shader.dispatch_accumulate_masked(*cov, 1, 4, BATCH, carry.data_ptr(), mask_tex), reps, trace, warmup)
            res[f"masked_1/{d}_over_plain"] = round(res[f"masked_1/{d}_ms"] / res["plain_ms"], 3)
        # the controller, on the state of a real frame after two batches
        guide, a, b = (rt.Texture.new_2d(r.ctx, W, H, bind=False) for _ in range(3))
        r.texture.clear()
        r.shader.dispatch_accumulate(*cov, 1, 0, BATCH)
        r.shader.dispatch_guide(guide)
        r.texture.adapt(guide, a, b, BATCH, TOL, r.adaptive_floor, 4, CAP)
        r.shader.dispatch_accumulate(*cov, 1, BATCH, BATCH)
        res["adapt_guide_ms"], res["adapt_guide_min_ms"] = windows(stream, lambda: r.texture.adapt(guide, b, a, BATCH, TOL, r.adaptive_floor, 4, CAP), reps, batch, warmup)
        res["adapt_counts"] = list(r.ctx.adapt_counts())
        res["adapt_ms"], res["adapt_min_ms"] = windows(stream, lambda: r.texture.adapt(None, b, a, BATCH, TOL, r.adaptive_floor, 4, CAP), reps, batch, warmup)
        scratch = rt.Texture.new_2d(r.ctx, W, H, bind=False)
        res["adapt_mean_ms"], res["adapt_mean_min_ms"] = windows(stream, lambda: scratch.adapt_mean(a), reps, batch, warmup)
        r.ctx.finish()
        for key, per_pixel in (("copy48", 48), ("copy64", 64)):
            src = torch.empty(per_pixel * W * H // 2, dtype=torch.uint8, device="cuda:0")
            dst = torch.empty_like(src)
            with torch.cuda.stream(stream):
                res[key + "_ms"], _ = windows(stream, lambda: dst.copy_(src), reps, batch, warmup)
        res["adapt_guide_over_copy64"] = round(res["adapt_guide_ms"] / res["copy64_ms"], 3)
        res["adapt_over_copy48"] = round(res["adapt_ms"] / res["copy48_ms"], 3)
        res["adapt_mean_over_copy48"] = round(res["adapt_mean_ms"] / res["copy48_ms"], 3)
        # the frame
        res["uniform_frame_ms"], res["uniform_frame_min_ms"] = windows(stream, lambda: r.render(), reps, 1, warmup)
        res["adaptive_frame_ms"], res["adaptive_frame_min_ms"] = windows(
            stream, lambda: r.render_adaptive(TOL, batch=BATCH, min_samples=4, max_samples=CAP), reps, 1, warmup)
        res["rounds"] = r.adaptive["rounds"]
        res["mean_spp"] = round(float(r.adaptive["samples"]().mean()), 3)
        res["adaptive_over_uniform"] = round(res["adaptive_frame_ms"] / res["uniform_frame_ms"], 3)
        res["adaptive_frame_batch8_ms"], _ = windows(stream, lambda: r.render_adaptive(TOL, batch=8, min_samples=4, max_samples=CAP), reps, 1, warmup)
        res["rounds_batch8"] = r.adaptive["rounds"]
        res["mean_spp_batch8"] = round(float(r.adaptive["samples"]().mean()), 3)
        return res
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_time_mi355x.txt"))
    args = ap.parse_args()
    lines = ["# tools/adaptive_time.py: ms per call, median (and min) over %d windows of %d calls (traces: %d; frames: 1, reads and the "
             "per-round count reads included); MI355X" % (args.reps, args.batch, max(1, args.batch // 4))]
    for name in POSES:
        line = json.dumps(time_scene(name, args.reps, args.batch, args.warmup))
        print(line, flush=True)
        lines.append(line)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
