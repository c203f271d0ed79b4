#!/usr/bin/env python3
"""Device-event timing of screen-space selection (csrc/tdt_select.hip), for the demo scene and scene config 1 at 1280x720 and
1920x1080, camera host.camera_reference_pose(W, H, 4, 6):

  tdt_dispatch_voxel_ids (place 0 and 1) beside tdt_dispatch_guide on the same frame in the same process: the same traversal, plus
  three fp64 divides per hit

  tdt_image_overlay at list sizes 0, 1, 2^10, 2^16 and 2^20 (the voxels the frame shows, padded with voxels drawn at random) for
  edge_width 0, 1 and 4, beside a device-to-device copy of the bytes the pass moves at most (16 B of ids per pixel read, 16 B of
  image read and written per member pixel: 48 B per pixel, which is what the copy moves, half read and half written).  The empty
  list is the pass alone (no upload, no sort, no member: 16 B per pixel read); a call with a list uploads it, with one host
  synchronisation, and queues keys, sort, unique and the pass, so from one voxel on the time holds that chain

  tdt_image_extract_voxels over the whole image (synchronous: pairs, sort, unique, read-back)

    python tools/select_time.py [--reps 15] [--batch 20] [--warmup 3] [--out profiles/select_time_mi355x.txt]

Every time is the median over `reps` windows of `batch` back-to-back calls between two HIP events on the context's stream, divided
by `batch`, after `warmup` untimed windows (lists of 2^16 and more, and the extraction: batch // 4).  Prints one JSON line per scene
and size and writes them to --out.  Measurement only: no test and no bench.py number depends on it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_time import windows  # noqa: E402

SPP = 4
SIZES = ((1280, 720), (1920, 1080))
LISTS = (0, 1, 1 << 10, 1 << 16, 1 << 20)
WIDTHS = (0, 1, 4)


def time_frame(name, scene, w, h, reps, batch, warmup):
    import torch
    from tdt4230_project_raytracing_amd import host, rt
    cam = host.camera_reference_pose(w, h, SPP, 6)
    stream = torch.cuda.Stream(device=0)
    r = rt.Renderer(scene, cam, stream=stream.cuda_stream)
    try:
        guide, ids = rt.Texture.new_2d(r.ctx, w, h, bind=False), rt.Texture.new_2d(r.ctx, w, h, bind=False)
        few = max(1, batch // 4)
        res = {"scene": name, "size": f"{w}x{h}", "reps": reps, "batch": batch}
        res["guide_ms"], res["guide_min_ms"] = windows(stream, lambda: r.shader.dispatch_guide(guide, all_materials=True), reps, batch, warmup)
        for place in (0, 1):
            res[f"ids_place{place}_ms"], res[f"ids_place{place}_min_ms"] = windows(stream, lambda: r.shader.dispatch_voxel_ids(ids, place), reps, batch, warmup)
        res["ids_over_guide"] = round(res["ids_place0_ms"] / res["guide_ms"], 3)
        r.shader.dispatch_voxel_ids(ids, 0)
        res["extract_ms"], res["extract_min_ms"] = windows(stream, lambda: ids.extract_voxels(), reps, few, warmup)
        seen = ids.extract_voxels()
        res["visible_voxels"] = len(seen)
        r.render()
        rng = np.random.default_rng(1)
        for n in LISTS:
            pad = np.concatenate([rng.integers(0, 1024, (max(n - len(seen), 0), 3)), np.ones((max(n - len(seen), 0), 1), np.int64)], 1).astype(np.int32)
            voxels = np.ascontiguousarray(np.concatenate([seen, pad])[:n])
            for ew in WIDTHS:
                key = f"overlay_n{n}_w{ew}"
                res[key + "_ms"], res[key + "_min_ms"] = windows(stream, lambda: r.texture.overlay(ids, voxels, (1, .6, 0, .35), (1, .6, 0, 1), ew),
                                                                 reps, batch if n < (1 << 16) else few, warmup)
            res[f"members_n{n}"] = round(r.ctx.overlay_counts()[2] / (w * h), 4)
        r.ctx.finish()
        src = torch.empty(24 * w * h, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        with torch.cuda.stream(stream):
            res["copy_ms"], res["copy_min_ms"] = windows(stream, lambda: dst.copy_(src), reps, batch, warmup)
        for ew in WIDTHS:
            res[f"overlay_n0_w{ew}_over_copy"] = round(res[f"overlay_n0_w{ew}_ms"] / res["copy_ms"], 3)
        return res
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_time_mi355x.txt"))
    args = ap.parse_args()
    from tdt4230_project_raytracing_amd import host
    lines = ["# tools/select_time.py: ms per call, median (and min) over %d windows of %d calls (lists of 2^16 and more, extraction: %d); MI355X"
             % (args.reps, args.batch, max(1, args.batch // 4))]
    for name, scene in (("demo", host.Scene.demo()), ("config1", host.Scene.config(1))):
        for w, h in SIZES:
            line = json.dumps(time_frame(name, scene, w, h, args.reps, args.batch, args.warmup))
            print(line, flush=True)
            lines.append(line)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
