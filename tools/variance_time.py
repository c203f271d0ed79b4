#!/usr/bin/env python3
"""Device-event timing of the variance unit (csrc/tdt_variance.hip) beside the calls it extends, on the same frames and in one
process:

  for the demo scene and scene config 1, at 1280x720 and 1920x1080, camera host.camera_reference_pose(W, H, 4, 6): tdt_image_variance
  (spatial estimate), tdt_image_denoise_variance with 1, 3 and 5 passes beside tdt_image_denoise with the same passes, and
  tdt_image_reproject_moments beside tdt_image_reproject, history from a frame yawed by one degree

    python tools/variance_time.py [--reps 15] [--batch 20] [--warmup 3] [--sigma 4] [--out profiles/variance_time_mi355x.txt]

The method is tools/denoise_time.py's: medians over `reps` windows of `batch` back-to-back calls between two HIP events on the
context's stream, after `warmup` untimed windows.  One difference, for both filters alike: a filter works in place, and twenty
variance-guided calls in a row would shrink the variance in alpha call after call until the luminance weight rejects nearly every
tap — not the work of a frame.  So every timed filter call is preceded by a device copy that restores the frame's sums (with their
variance), the copy alone is timed the same way, and the figures reported are the differences (the raw ones are kept as *_raw_ms).
The existing calls are the yardstick.  Measurement only: no test and no bench.py number depends on it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_time import windows  # noqa: E402
from reproject_time import cover, yaw_units  # noqa: E402


def time_frame(name, scene, w, h, reps, batch, warmup, sigma):
    import torch
    from tdt4230_project_raytracing_amd import host, rt
    spp = 4
    cam = host.camera_reference_pose(w, h, spp, 6)
    stream = torch.cuda.Stream(device=0)
    image = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r = rt.Renderer(scene, cam, stream=stream.cuda_stream, image_ptr=image.data_ptr())
    try:
        new = lambda: rt.Texture.new_2d(r.ctx, w, h, bind=False)  # noqa: E731
        guide, old_guide, hist, old_hist, mean, moments, old_moments = new(), new(), new(), new(), new(), new(), new()
        res = {"scene": name, "size": f"{w}x{h}", "spp": spp, "reps": reps, "batch": batch, "sigma": sigma}
        # the earlier frame: the same camera yawed back by one degree, its guide, its first history and its first moments
        turned = host.Camera(90.0, w, aspect_ratio=np.float32(w) / np.float32(h), origin=list(cam.origin), viewport_height=2.0,
                             samples_per_pixel=spp, max_bounce=6)
        here = turned.uniforms()
        turned.turn_yaw(yaw_units(turned, -1.0))
        rt.initial_uniforms(turned.uniforms(), r.shader.program)
        r.shader.dispatch_accumulate(*cover(w, h), 1, 0, spp)
        r.shader.dispatch_guide(old_guide)
        r.texture.reproject_moments(r.shader, 0, old_guide, spp, hist_out=old_hist, moments_out=old_moments)
        old_view = r.shader.view()
        rt.initial_uniforms(here, r.shader.program)
        r.texture.clear()
        r.shader.dispatch_accumulate(*cover(w, h), 1, spp, spp)
        r.shader.dispatch_guide(guide, sample=spp)
        prev = (old_view, old_guide, old_hist)
        res["reproject_ms"], res["reproject_min_ms"] = windows(
            stream, lambda: r.texture.reproject(r.shader, spp, guide, spp, prev, 64.0, hist_out=hist, mean_out=mean), reps, batch, warmup)
        res["reproject_moments_ms"], res["reproject_moments_min_ms"] = windows(
            stream, lambda: r.texture.reproject_moments(r.shader, spp, guide, spp, prev + (old_moments,), 64.0, hist_out=hist, moments_out=moments,
                                                        mean_out=mean), reps, batch, warmup)
        counts = r.ctx.reproject_counts()
        res["keyed_fraction"] = round(counts[0] / (w * h), 4)
        res["found_of_keyed"] = round(counts[1] / max(1, counts[0]), 4)
        # the variance: it writes alpha alone, so it repeats on the same input
        res["variance_ms"], res["variance_min_ms"] = windows(stream, lambda: r.texture.variance(guide), reps, batch, warmup)
        r.ctx.finish()
        saved = image.clone()                                         # the sums with their variance: what every filter call starts from
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            restore = lambda: image.copy_(saved)  # noqa: E731
            res["restore_ms"], _ = windows(stream, restore, reps, batch, warmup)
            for passes in (1, 3, 5):
                for key, call in (("denoise", lambda: r.texture.denoise(guide, passes)),
                                  ("denoise_variance", lambda: r.texture.denoise_variance(guide, passes, sigma))):
                    raw, raw_min = windows(stream, lambda: (restore(), call()), reps, batch, warmup)
                    res[f"{key}{passes}_raw_ms"] = raw
                    res[f"{key}{passes}_ms"] = round(raw - res["restore_ms"], 4)
                res[f"variance_over_key_only_{passes}"] = round(res[f"denoise_variance{passes}_ms"] / res[f"denoise{passes}_ms"], 3)
        res["reproject_moments_over_reproject"] = round(res["reproject_moments_ms"] / res["reproject_ms"], 3)
        r.ctx.finish()
        return res
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance_time_mi355x.txt"))
    args = ap.parse_args()
    from tdt4230_project_raytracing_amd import host
    lines = ["# tools/variance_time.py: ms per call, median (and min) over %d windows of %d calls; MI355X; filter calls net of the"
             " restoring copy (restore_ms), raw figures beside them" % (args.reps, args.batch)]
    for name, scene in (("demo", host.Scene.demo()), ("config1", host.Scene.config(1))):
        for w, h in ((1280, 720), (1920, 1080)):
            line = json.dumps(time_frame(name, scene, w, h, args.reps, args.batch, args.warmup, args.sigma))
            print(line, flush=True)
            lines.append(line)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
