#!/usr/bin/env python3
"""Device-event timing of temporal reprojection (csrc/tdt_reproject.hip) beside the frame it extends, and what it buys:

  timing, for the demo scene and scene config 1 at 1280x720 and 1920x1080, camera host.camera_reference_pose(W, H, 4, 6):
  tdt_image_reproject with the history of a frame yawed by one degree (yaw_units converts; mean written in place), beside that run's 4-spp trace
  (tdt_dispatch_compute), tdt_dispatch_guide, three passes of tdt_image_denoise, and a device-to-device copy that moves the same
  96 B per pixel (48 B read and 48 B written per pixel; the call reads guide, sums, old guide, old history and writes history and
  mean, 16 B each) — the floor a memory-bound gather is judged against

  quality (--quality), at 1280x720 over a turn of 16 frames of one degree each: RMSE of the resolved frame against a 1024-spp frame
  of the same view, mean over the 16 frames and of the last one, for the plain 4-spp frame, denoise=3, render_temporal and
  render_temporal with denoise=3, with the found / rejected fractions of tdt_debug_reproject_counts over frames 1..15

    python tools/reproject_time.py [--reps 15] [--batch 20] [--warmup 3] [--quality] [--out profiles/reproject_time_mi355x.txt]

Every time is the median over `reps` windows of `batch` back-to-back calls between two HIP events on the context's stream, divided
by `batch`, after `warmup` untimed windows.  Prints one JSON line per scene and size and writes them to --out.  Measurement only:
no test and no bench.py number depends on it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_time import windows  # noqa: E402


def yaw_units(camera, degrees):
    """`degrees` in the units of host.Camera.turn_yaw, which rotates by 2 * angle * turn_rate radians (camera.rs:56-62)."""
    return float(np.radians(degrees)) / (2.0 * camera.c.settings.turn_rate)


def cover(w, h):
    return -(-w // 32) * 32, -(-h // 32) * 32


def time_frame(name, scene, w, h, reps, batch, warmup):
    import torch
    from tdt4230_project_raytracing_amd import host, rt
    spp = 4
    cam = host.camera_reference_pose(w, h, spp, 6)
    stream = torch.cuda.Stream(device=0)
    r = rt.Renderer(scene, cam, stream=stream.cuda_stream)
    try:
        new = lambda: rt.Texture.new_2d(r.ctx, w, h, bind=False)  # noqa: E731
        guide, old_guide, hist, old_hist = new(), new(), new(), new()
        res = {"scene": name, "size": f"{w}x{h}", "spp": spp, "reps": reps, "batch": batch}
        res["trace_ms"], res["trace_min_ms"] = windows(stream, r.dispatch, reps, max(1, batch // 4), warmup)
        res["guide_ms"], res["guide_min_ms"] = windows(stream, lambda: r.shader.dispatch_guide(guide), reps, batch, warmup)
        # the earlier frame: the same camera yawed back by one degree, its guide and its first history
        turned = host.Camera(90.0, w, aspect_ratio=np.float32(w) / np.float32(h), origin=list(cam.origin), viewport_height=2.0,
                             samples_per_pixel=spp, max_bounce=6)
        here = turned.uniforms()
        turned.turn_yaw(yaw_units(turned, -1.0))
        rt.initial_uniforms(turned.uniforms(), r.shader.program)
        r.shader.dispatch_accumulate(*cover(w, h), 1, 0, spp)
        r.shader.dispatch_guide(old_guide)
        r.texture.reproject(r.shader, 0, old_guide, spp, hist_out=old_hist)
        old_view = r.shader.view()
        rt.initial_uniforms(here, r.shader.program)
        r.texture.clear()
        r.shader.dispatch_accumulate(*cover(w, h), 1, spp, spp)
        r.shader.dispatch_guide(guide, sample=spp)
        call = lambda: r.texture.reproject(r.shader, spp, guide, spp, (old_view, old_guide, old_hist), 64.0, hist_out=hist, mean_out=r.texture)  # noqa: E731
        res["reproject_ms"], res["reproject_min_ms"] = windows(stream, call, reps, batch, warmup)
        counts = r.ctx.reproject_counts()
        res["keyed_fraction"] = round(counts[0] / (w * h), 4)
        res["found_of_keyed"] = round(counts[1] / max(1, counts[0]), 4)
        res["denoise3_ms"], res["denoise3_min_ms"] = windows(stream, lambda: r.texture.denoise(guide, 3), reps, batch, warmup)
        r.ctx.finish()
        src = torch.empty(w * h * 48, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        with torch.cuda.stream(stream):
            res["copy96_ms"], res["copy96_min_ms"] = windows(stream, lambda: dst.copy_(src), reps, batch, warmup)
        res["reproject_over_copy96"] = round(res["reproject_ms"] / res["copy96_ms"], 3)
        res["reproject_over_trace"] = round(res["reproject_ms"] / res["trace_ms"], 3)
        res["reproject_GBps"] = round(w * h * 96 / (res["reproject_ms"] * 1e-3) / 1e9, 1)
        return res
    finally:
        r.close()


# (origin, yaw, pitch, vertical fov): yaw and pitch of the first frame in controller units (turn_yaw / turn_pitch of a default
# host.Camera: 2 * 0.025 rad = 2.865 degrees each), not degrees; the turn from there on is in degrees through yaw_units
POSES = {"config1": ((0.1, 0.05, -0.6), 135.0, 10.0, 70.0), "demo": ((0.0, 0.2, 0.9), -8.0, -8.0, 90.0)}


def quality(name, scene, w=1280, h=720, frames=16, spp=4, ref_spp=1024, degrees=1.0):
    from tdt4230_project_raytracing_amd import host, rt
    origin, yaw, pitch, fov = POSES[name]
    cams = []
    for k in range(frames):
        c = host.Camera(fov, w, aspect_ratio=np.float32(w) / np.float32(h), origin=list(origin), viewport_height=2.0, samples_per_pixel=spp,
                        max_bounce=6)
        c.turn_yaw(yaw + yaw_units(c, k * degrees))
        c.turn_pitch(pitch)
        cams.append(c.uniforms())
    cov = cover(w, h)
    plain_r, temporal_r, both_r = (rt.Renderer(scene, cams[0]) for _ in range(3))
    err = {"plain": [], "denoise3": [], "temporal": [], "temporal_denoise3": []}
    counts = np.zeros(4, np.int64)
    try:
        for k, cam in enumerate(cams):
            plain_r.camera = cam
            rt.initial_uniforms(cam, plain_r.shader.program)
            plain_r.shader.dispatch_accumulate(*cov, 1, 0, ref_spp)
            plain_r.shader.dispatch_resolve(*cov, 1, ref_spp)
            ref = plain_r.texture.read()[..., :3].astype(np.float64)
            rmse = lambda img: float(np.sqrt(np.mean((img[..., :3] - ref) ** 2)))  # noqa: E731
            err["plain"].append(rmse(plain_r.render(*cov)))
            err["denoise3"].append(rmse(plain_r.render(*cov, denoise=3)))
            err["temporal"].append(rmse(temporal_r.render_temporal(*cov, cam=cam)))
            if k:
                counts += np.array(temporal_r.ctx.reproject_counts(), np.int64)
            err["temporal_denoise3"].append(rmse(both_r.render_temporal(*cov, cam=cam, denoise=3)))
    finally:
        for r in (plain_r, temporal_r, both_r):
            r.close()
    res = {"scene": name, "size": f"{w}x{h}", "frames": frames, "degrees_per_frame": degrees, "spp": spp, "reference_spp": ref_spp, "max_samples": 64}
    for k, v in err.items():
        res[f"rmse_{k}_mean"], res[f"rmse_{k}_last"] = round(float(np.mean(v)), 5), round(v[-1], 5)
    keyed = max(1, int(counts[0]))
    res["keyed_fraction"] = round(int(counts[0]) / ((frames - 1) * w * h), 4)
    res["found_of_keyed"], res["rejected_by_key_of_keyed"], res["off_screen_of_keyed"] = (round(int(c) / keyed, 4) for c in counts[1:])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_time_mi355x.txt"))
    args = ap.parse_args()
    from tdt4230_project_raytracing_amd import host
    lines = ["# tools/reproject_time.py: ms per call, median (and min) over %d windows of %d calls; MI355X" % (args.reps, args.batch)]
    scenes = (("demo", host.Scene.demo()), ("config1", host.Scene.config(1)))
    for name, scene in scenes:
        for w, h in ((1280, 720), (1920, 1080)):
            line = json.dumps(time_frame(name, scene, w, h, args.reps, args.batch, args.warmup))
            print(line, flush=True)
            lines.append(line)
    if args.quality:
        lines.append("# quality: RMSE of resolved frames against 1024 spp over a turn of 16 frames, one degree each")
        for name, scene in scenes:
            line = json.dumps(quality(name, scene))
            print(line, flush=True)
            lines.append(line)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
