#!/usr/bin/env python3
"""Device-event timing of guide-keyed upsampling (csrc/tdt_upsample.hip) beside the frame it replaces, and what the frame loses:

  timing, for the demo scene and scene config 1 at 1280x720 and 1920x1080, 4 spp, camera host.camera_reference_pose(W, H, 4, 6), at
  scales 2 and 3: the full-resolution trace (tdt_dispatch_compute), and the pieces of Renderer.render_upsampled — the low trace
  (tdt_dispatch_accumulate under image_width = ceil(W / scale), image_height = ceil(H / scale)), the low and the full guide,
  tdt_image_upsample, the resolve — each alone and as the whole chain in one window; and a device-to-device copy that moves the
  call's own bytes (32 B per pixel of the full image and 32 B per texel of the low one, half of them read and half written) — the
  floor a memory-bound gather is judged against

  quality, same scenes and sizes, poses of tools/reproject_time.py: RMSE of the resolved frame against a 1024-spp frame of the same
  view, for render() and render_upsampled(scale), without a filter and with denoise=3, and the class counts of
  tdt_debug_upsample_counts

    python tools/upsample_time.py [--reps 15] [--batch 20] [--warmup 3] [--no-quality] [--out profiles/upsample_time_mi355x.txt]

Every time is the median over `reps` windows of `batch` back-to-back calls between two HIP events on the context's stream, divided
by `batch`, after `warmup` untimed windows.  Prints one JSON line per scene, size and scale and writes them to --out.  Measurement
only: no test and no bench.py number depends on it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_time import windows  # noqa: E402
from reproject_time import POSES, cover  # noqa: E402

SPP = 4
SCALES = (2, 3)
SIZES = ((1280, 720), (1920, 1080))


def time_frame(name, scene, w, h, reps, batch, warmup):
    import torch
    from tdt4230_project_raytracing_amd import host, rt
    cam = host.camera_reference_pose(w, h, SPP, 6)
    stream = torch.cuda.Stream(device=0)
    r = rt.Renderer(scene, cam, stream=stream.cuda_stream)
    out = []
    try:
        program = r.shader.program
        guide = rt.Texture.new_2d(r.ctx, w, h, bind=False)
        trace = max(1, batch // 4)
        full_ms, full_min = windows(stream, lambda: r.shader.dispatch_compute(*cover(w, h), 1), reps, trace, warmup)   # (all rows, as the chain)
        guide_ms, _ = windows(stream, lambda: r.shader.dispatch_guide(guide), reps, batch, warmup)
        resolve_ms, _ = windows(stream, lambda: r.shader.dispatch_resolve(*cover(w, h), 1, SPP), reps, batch, warmup)
        for scale in SCALES:
            lw, lh = -(-w // scale), -(-h // scale)
            low, low_guide = rt.Texture.new_2d(r.ctx, lw, lh, bind=False), rt.Texture.new_2d(r.ctx, lw, lh, bind=False)

            def low_uniforms():
                program.set_i32("camera.image_width", lw)
                program.set_i32("camera.image_height", lh)
                low.bind()

            def full_uniforms():
                program.set_i32("camera.image_width", w)
                program.set_i32("camera.image_height", h)
                r.texture.bind()

            def chain():
                low_uniforms()
                r.shader.dispatch_accumulate(*cover(lw, lh), 1, 0, SPP)
                r.shader.dispatch_guide(low_guide)
                full_uniforms()
                r.shader.dispatch_guide(guide)
                r.texture.upsample(guide, low, low_guide)
                r.shader.dispatch_resolve(*cover(w, h), 1, SPP)
            res = {"scene": name, "size": f"{w}x{h}", "scale": scale, "low": f"{lw}x{lh}", "spp": SPP, "reps": reps, "batch": batch,
                   "full_trace_ms": full_ms, "full_trace_min_ms": full_min, "full_guide_ms": guide_ms, "resolve_ms": resolve_ms}
            low_uniforms()
            res["low_trace_ms"], res["low_trace_min_ms"] = windows(stream, lambda: r.shader.dispatch_accumulate(*cover(lw, lh), 1, 0, SPP), reps, trace, warmup)
            res["low_guide_ms"], _ = windows(stream, lambda: r.shader.dispatch_guide(low_guide), reps, batch, warmup)
            full_uniforms()
            r.shader.dispatch_guide(guide)
            res["upsample_ms"], res["upsample_min_ms"] = windows(stream, lambda: r.texture.upsample(guide, low, low_guide), reps, batch, warmup)
            counts = r.ctx.upsample_counts()
            res["bilinear"], res["ring"], res["holes"] = (round(c / counts[0], 4) for c in counts[1:])
            res["frame_upsampled_ms"], res["frame_upsampled_min_ms"] = windows(stream, chain, reps, trace, warmup)
            r.ctx.finish()
            call_bytes = 32 * (w * h + lw * lh)
            src = torch.empty(call_bytes // 2, dtype=torch.uint8, device="cuda:0")
            dst = torch.empty_like(src)
            with torch.cuda.stream(stream):
                res["copy_ms"], res["copy_min_ms"] = windows(stream, lambda: dst.copy_(src), reps, batch, warmup)
            res["upsample_over_copy"] = round(res["upsample_ms"] / res["copy_ms"], 3)
            res["upsample_GBps"] = round(call_bytes / (res["upsample_ms"] * 1e-3) / 1e9, 1)
            res["sum_of_parts_ms"] = round(res["low_trace_ms"] + res["low_guide_ms"] + guide_ms + res["upsample_ms"] + resolve_ms, 4)
            res["frame_upsampled_over_full_trace"] = round(res["frame_upsampled_ms"] / full_ms, 3)
            out.append(res)
        return out
    finally:
        r.close()


def quality(name, scene, w, h, ref_spp=1024):
    from tdt4230_project_raytracing_amd import host, rt
    origin, yaw, pitch, fov = POSES[name]
    c = host.Camera(fov, w, aspect_ratio=np.float32(w) / np.float32(h), origin=list(origin), viewport_height=2.0, samples_per_pixel=SPP, max_bounce=6)
    c.turn_yaw(yaw)
    c.turn_pitch(pitch)
    cov = cover(w, h)
    r = rt.Renderer(scene, c.uniforms())
    try:
        r.shader.dispatch_accumulate(*cov, 1, 0, ref_spp)
        r.shader.dispatch_resolve(*cov, 1, ref_spp)
        ref = r.texture.read()[..., :3].astype(np.float64)
        rmse = lambda img: round(float(np.sqrt(np.mean((img[..., :3] - ref) ** 2))), 5)  # noqa: E731
        res = {"scene": name, "size": f"{w}x{h}", "spp": SPP, "reference_spp": ref_spp,
               "rmse_full": rmse(r.render(*cov)), "rmse_full_denoise3": rmse(r.render(*cov, denoise=3))}
        for scale in SCALES:
            res[f"rmse_scale{scale}"] = rmse(r.render_upsampled(scale, 0, *cov))
            counts = r.ctx.upsample_counts()
            res[f"classes_scale{scale}"] = [round(v / counts[0], 4) for v in counts[1:]]
            res[f"holes_scale{scale}"] = counts[3]
            res[f"rmse_scale{scale}_denoise3"] = rmse(r.render_upsampled(scale, 3, *cov))
        return res
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_time_mi355x.txt"))
    args = ap.parse_args()
    from tdt4230_project_raytracing_amd import host
    lines = ["# tools/upsample_time.py: ms per call, median (and min) over %d windows of %d calls (traces and whole frames: %d); MI355X"
             % (args.reps, args.batch, max(1, args.batch // 4))]
    scenes = (("demo", host.Scene.demo()), ("config1", host.Scene.config(1)))
    for name, scene in scenes:
        for w, h in SIZES:
            for res in time_frame(name, scene, w, h, args.reps, args.batch, args.warmup):
                line = json.dumps(res)
                print(line, flush=True)
                lines.append(line)
    if not args.no_quality:
        lines.append("# quality: RMSE of resolved frames against 1024 spp of the same view; classes = bilinear, ring, holes as shares of the pixels")
        for name, scene in scenes:
            for w, h in SIZES:
                line = json.dumps(quality(name, scene, w, h))
                print(line, flush=True)
                lines.append(line)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
