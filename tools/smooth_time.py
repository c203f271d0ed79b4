#!/usr/bin/env python3
"""Voxel smoothing on the GPU (tdt_octree_smooth): host wall-clock medians after warm-up on configs 3 and 5 — the majority filter
with border 1 at squared radius 3, 16 and 225, 1 and 4 iterations, as the preview (tdt_octree_extract_smooth, which runs the
filter twice: count, then fill) and as the edit — each alternating, call by call, with two baselines that see the same machine
state: tdt_octree_morph_round's DILATE at the same squared radius (the yardstick: one distance transform where this unit runs a
windowed popcount per iteration) and tdt_octree_compact of the same tree (the rebuild every edit pays).  Every timed result is
checked against the numpy model (tests/smooth_model.py) on trees up to --check-depth and radii up to --check-radius2 (the model's
chord loop over a depth-8 grid at radius2 225 takes minutes); the others are reported as unchecked.

    python tools/smooth_time.py [--reps N] [--warmup N] [--configs 3,5] [--radii2 3,16,225] [--iterations 1,4] [--check-depth 8]
                                [--check-radius2 16]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import smooth_model as sm  # noqa: E402
from distance_model import window_of  # noqa: E402
from test_gpu_region_edit import built_cells, padded  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402


def timed(fns, reset, reps, warmup):
    """Medians of the functions, called in turn (reset() before each, not timed; every call synchronises)."""
    ts = [[] for _ in fns]
    for i in range(warmup + reps):
        for fn, t in zip(fns, ts):
            reset()
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                t.append(time.perf_counter() - t0)
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--radii2", default="3,16,225")
    ap.add_argument("--iterations", default="1,4")
    ap.add_argument("--check-depth", type=int, default=8)
    ap.add_argument("--check-radius2", type=int, default=16)
    a = ap.parse_args()
    all_ok = True
    for cfg in [int(c) for c in a.configs.split(",")]:
        scene = host.Scene.config(cfg)
        depth = scene.max_depth
        orig = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
        ctx = rt.Context(0)
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        print(f"config {cfg}: depth {depth}, {len(V)} voxels, {len(orig) // 16} cells", flush=True)
        for r2 in [int(r) for r in a.radii2.split(",")]:
            for it in [int(i) for i in a.iterations.split(",")]:
                kw = dict(radius2=r2, iterations=it, border=1)
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, vbos[0])          # the previews are of the scene's own tree
                preview = ctx.octree_extract_smooth(**kw)
                grown = ctx.octree_extract_morph_round(rt.MORPH_DILATE, r2, material=7)
                room = max(len(orig), len(built_cells(ctx, preview, depth, model=False)), len(built_cells(ctx, grown, depth, model=False))) // 16 + 8
                start = padded(orig, 64 * room)
                buf = rt.VertexBufferObject(ctx, start)
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)

                def reset():
                    buf.sub_data(0, start)
                    ctx.finish()

                rnd, base, pre, m = timed([lambda: ctx.octree_morph_round(rt.MORPH_DILATE, r2, material=7), ctx.octree_compact,
                                           lambda: ctx.octree_extract_smooth(**kw), lambda: ctx.octree_smooth(**kw)], reset, a.reps, a.warmup)
                after = ctx.octree_extract()
                verdict = "unchecked"
                if depth <= a.check_depth and r2 <= a.check_radius2:
                    ok = np.array_equal(after, sm.smooth(V, depth, **kw))
                    all_ok &= ok
                    verdict = "matches numpy" if ok else "DIFFERS from numpy"
                if not np.array_equal(preview, after):
                    all_ok, verdict = False, "the preview DIFFERS from the edit"
                print(f"  radius2 {r2:3d} (R {window_of(r2):2d}) x{it}  edit {m * 1e3:8.2f} ms  preview {pre * 1e3:8.2f} ms  round DILATE {rnd * 1e3:8.2f} ms  "
                      f"compact {base * 1e3:7.2f} ms  ({m / rnd:5.2f}x round)  {len(preview):>9d} voxels  {verdict}", flush=True)
                del buf
        del vbos
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
