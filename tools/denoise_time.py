#!/usr/bin/env python3
"""Device-event timing of the guide launch and the denoiser (csrc/tdt_denoise.hip) beside the frame they clean:

  for the demo scene and scene config 1, at 1280x720 and 1920x1080, camera host.camera_reference_pose(W, H, 4, 6) — the 4-spp
  frame the reference's main.rs asks for —: tdt_dispatch_guide, tdt_image_denoise with 1, 3 and 5 passes, and the 4-spp trace
  (tdt_dispatch_compute) of the same frame

    python tools/denoise_time.py [--reps 15] [--batch 20] [--warmup 3] [--out profiles/denoise_time_mi355x.txt]

Every figure is the median over `reps` windows of `batch` back-to-back calls between two HIP events on the context's stream,
divided by `batch` (a single filter pass is far shorter than what an event pair resolves well), after `warmup` untimed windows.
The filter runs in place on the frame's running sums; the trace is timed on frames that repeat their inputs (the one-pass
schedule).  Prints one JSON line per scene and size and writes them to --out.  Measurement only: no test and no bench.py number
depends on it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(stream, call, reps, batch, warmup):
    """(median, min) ms per call."""
    import torch
    ms = []
    for k in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(batch):
            call()
        b.record(stream)
        b.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b) / batch)
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def time_frame(name, scene, w, h, reps, batch, warmup):
    import torch
    from tdt4230_project_raytracing_amd import host, rt
    spp = 4
    cam = host.camera_reference_pose(w, h, spp, 6)
    stream = torch.cuda.Stream(device=0)
    r = rt.Renderer(scene, cam, stream=stream.cuda_stream)
    try:
        guide = rt.Texture.new_2d(r.ctx, w, h, bind=False)
        res = {"scene": name, "size": f"{w}x{h}", "spp": spp, "reps": reps, "batch": batch}
        res["trace_ms"], res["trace_min_ms"] = windows(stream, r.dispatch, reps, max(1, batch // 4), warmup)
        res["guide_ms"], res["guide_min_ms"] = windows(stream, lambda: r.shader.dispatch_guide(guide), reps, batch, warmup)
        r.shader.dispatch_accumulate(w + 1, h + 1, 1, 0, spp)          # the sums the filter is meant for
        for passes in (1, 3, 5):
            res[f"denoise{passes}_ms"], res[f"denoise{passes}_min_ms"] = windows(stream, lambda: r.texture.denoise(guide, passes), reps, batch, warmup)
        r.ctx.finish()
        g = guide.read_guide()
        res["pass_through_fraction"] = round(float((g["kind"] == 0).mean()), 4)
        for passes in (1, 3, 5):
            res[f"guide_plus_denoise{passes}_over_trace"] = round((res["guide_ms"] + res[f"denoise{passes}_ms"]) / res["trace_ms"], 3)
        return res
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_time_mi355x.txt"))
    args = ap.parse_args()
    from tdt4230_project_raytracing_amd import host
    lines = ["# tools/denoise_time.py: ms per call, median (and min) over %d windows of %d calls; MI355X" % (args.reps, args.batch)]
    for name, scene in (("demo", host.Scene.demo()), ("config1", host.Scene.config(1))):
        for w, h in ((1280, 720), (1920, 1080)):
            line = json.dumps(time_frame(name, scene, w, h, args.reps, args.batch, args.warmup))
            print(line, flush=True)
            lines.append(line)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
