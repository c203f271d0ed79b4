#!/usr/bin/env python3
"""Device-event timing of through-selection (csrc/tdt_screen.hip) on scene config 1 and on the largest voxel list of
tests/tree_cases.py, at 1280x720:

  tdt_octree_extract_screen for a rectangle (the middle half of the image), a 3-vertex and a 256-vertex polygon (a triangle and a fine
  circle over the same area) and a mask (the rectangle, painted), each with the centre rule and with TDT_SCREEN_WINDOW

  tdt_octree_extract_region of a whole-grid box on the same tree beside them: both calls pay the same walk of the tree, the same
  scan, gather and host synchronisations, so the difference is the predicate's cost

    python tools/screen_select_time.py [--reps 15] [--batch 10] [--warmup 3] [--out profiles/screen_select_time_mi355x.txt]

Both calls are synchronous, so a time holds the host's part too.  Every call is made with a NULL array (the count alone: no list is
copied to the host, whose size would differ between the two); "list" rows add the copy for the rectangle and the box, and
"region_count_again" repeats the box behind everything else (the drift within the process).  Every time is the
median over `reps` windows of `batch` back-to-back calls between two HIP events on the context's stream, divided by `batch`, after
`warmup` untimed windows.  Prints one JSON line per tree and writes them to --out.  Measurement only: no test and no bench.py number
depends on it."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from denoise_time import windows  # noqa: E402

W, H = 1280, 720


def shapes():
    x0, y0, x1, y1 = W // 4, H // 4, 3 * W // 4, 3 * H // 4
    t = 2 * np.pi * np.arange(256) / 256
    circle = np.stack([W / 2 + H / 3 * np.cos(t), H / 2 + H / 3 * np.sin(t)], 1).round().astype(np.int32)
    mask = np.zeros((H, W, 4), np.float32)
    mask[y0: y1 + 1, x0: x1 + 1, 0] = 1.0
    return {"rect": dict(rect=(x0, y0, x1, y1)), "poly3": dict(polygon=np.array([(x0, y0), (x1, y0), (W // 2, y1)], np.int32)),
            "poly256": dict(polygon=circle), "mask": dict(mask=mask)}


def time_tree(name, ctx, stream, view, n_voxels, reps, batch, warmup):
    import torch
    from tdt4230_project_raytracing_amd import rt
    L = rt.lib()
    res = {"tree": name, "size": f"{W}x{H}", "voxels": n_voxels, "reps": reps, "batch": batch}
    n = ctypes.c_size_t(0)
    out = np.zeros((max(n_voxels, 1), 4), np.int32)
    grid = rt.box((0, 0, 0), (1023, 1023, 1023))

    def region(array):
        ctx.check(L.tdt_octree_extract_region(ctx.h, ctypes.byref(grid), 1, out.ctypes.data if array else None, len(out) if array else 0, ctypes.byref(n)))

    res["region_count_ms"], res["region_count_min_ms"] = windows(stream, lambda: region(False), reps, batch, warmup)
    res["region_list_ms"], res["region_list_min_ms"] = windows(stream, lambda: region(True), reps, batch, warmup)
    keep = []
    for shape, kw in shapes().items():
        if "mask" in kw:
            t = torch.from_numpy(kw["mask"]).to("cuda:0")
            torch.cuda.synchronize()
            keep.append(t)
            kw = dict(mask=rt.Texture.wrap_device(ctx, t.data_ptr(), W, H, bind=False))
        for window in (False, True):
            sel, pts, mask = rt._screen_select(kw.get("rect"), kw.get("polygon"), kw.get("mask"), window, None, 0.0, float("inf"))

            def screen(array):
                ctx.check(L.tdt_octree_extract_screen(ctx.h, ctypes.byref(view), ctypes.byref(sel), pts.ctypes.data if pts is not None else None,
                                                      len(pts) if pts is not None else 0, mask.h if mask is not None else None,
                                                      out.ctypes.data if array else None, len(out) if array else 0, ctypes.byref(n)))

            key = f"{shape}_{'window' if window else 'centre'}"
            res[key + "_ms"], res[key + "_min_ms"] = windows(stream, lambda: screen(False), reps, batch, warmup)
            res[key + "_selected"] = ctx.screen_counts()[3]
            res[key + "_over_region"] = round(res[key + "_ms"] / res["region_count_ms"], 3)
            if shape == "rect":
                res[key + "_list_ms"], res[key + "_list_min_ms"] = windows(stream, lambda: screen(True), reps, batch, warmup)
    # the box once more, behind everything else: the drift of the process over the run, which bounds what a difference above means
    res["region_count_again_ms"], res["region_count_again_min_ms"] = windows(stream, lambda: region(False), reps, batch, warmup)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_select_time_mi355x.txt"))
    args = ap.parse_args()
    import torch
    import tree_cases
    from tdt4230_project_raytracing_amd import host, rt
    lines = ["# tools/screen_select_time.py: ms per call, median (and min) over %d windows of %d calls; MI355X" % (args.reps, args.batch)]
    stream = torch.cuda.Stream(device=0)
    # scene config 1 under the reference camera
    r = rt.Renderer(host.Scene.config(1), host.camera_reference_pose(W, H, 4, 6), stream=stream.cuda_stream)
    try:
        lines.append(json.dumps(time_tree("config1", r.ctx, stream, r.shader.view(), len(r.ctx.octree_extract()), args.reps, args.batch, args.warmup)))
        print(lines[-1], flush=True)
    finally:
        r.close()
    # the largest list of tests/tree_cases.py in the unit cube, seen from in front of it
    name, depth, vox = max(tree_cases.families(), key=lambda f: len(f[2]))
    ctx = rt.Context(0, stream.cuda_stream)
    try:
        cells, _ = rt.octree_build_cells(ctx, np.ascontiguousarray(vox, np.int32), depth)
        floats = rt.VertexBufferObject(ctx, np.array([0, 0, 0, 0, 1, 1, 1 / 64], np.float32))
        ints = rt.VertexBufferObject(ctx, np.array([depth, 64, 64], np.int32))
        for slot, b in ((0, cells), (6, floats), (7, ints)):
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, slot, b)
        view = rt.VIEW((ctypes.c_float * 3)(0.5, 0.5, -1.0), (ctypes.c_float * 3)(-0.3, 0.05, 0.0), (ctypes.c_float * 3)(1.6, 0, 0),
                       (ctypes.c_float * 3)(0, 0.9, 0), W, H)
        lines.append(json.dumps(time_tree(name, ctx, stream, view, len(vox), args.reps, args.batch, args.warmup)))
        print(lines[-1], flush=True)
    finally:
        ctx.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
