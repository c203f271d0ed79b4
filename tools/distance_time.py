#!/usr/bin/env python3
"""Round morphology on the GPU (tdt_octree_morph_round): host wall-clock medians after warm-up on configs 3 and 5 — DILATE, ERODE
and CLOSE at squared radius 1, 16 and 256 — each alternating, call by call, with two baselines that see the same machine state:
the step-wise tdt_octree_morph at connectivity 26 with the same R steps, and tdt_octree_compact of the same tree (the rebuild
every edit pays).  Every timed round result is checked against the numpy model (tests/distance_model.py) on trees up to
--check-depth (the dense model needs 8 bytes x a few copies per grid voxel: gigabytes and minutes at depth 9); deeper trees are
reported as unchecked.

    python tools/distance_time.py [--reps N] [--warmup N] [--configs 3,5] [--radii2 1,16,256] [--check-depth 8]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import distance_model as dm  # noqa: E402
from test_gpu_region_edit import built_cells, padded  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402

OPS = (("DILATE", rt.MORPH_DILATE), ("ERODE", rt.MORPH_ERODE), ("CLOSE", rt.MORPH_CLOSE))


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
    ap.add_argument("--radii2", default="1,16,256")
    ap.add_argument("--check-depth", type=int, default=8)
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
        for name, op in OPS:
            for r2 in [int(r) for r in a.radii2.split(",")]:
                R = dm.window_of(r2)
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, vbos[0])          # the previews are of the scene's own tree
                preview = ctx.octree_extract_morph_round(op, r2, material=7)
                steps = ctx.octree_extract_morph(op, R, 26, material=7)                 # the cube of the same R: the larger result
                room = max(len(orig), len(built_cells(ctx, preview, depth, model=False)), len(built_cells(ctx, steps, depth, model=False))) // 16 + 8
                start = padded(orig, 64 * room)
                buf = rt.VertexBufferObject(ctx, start)
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)

                def reset():
                    buf.sub_data(0, start)
                    ctx.finish()

                step, base, m = timed([lambda: ctx.octree_morph(op, R, 26, material=7), ctx.octree_compact,
                                       lambda: ctx.octree_morph_round(op, r2, material=7)], reset, a.reps, a.warmup)
                verdict = "unchecked"
                if depth <= a.check_depth:
                    ok = np.array_equal(ctx.octree_extract(), dm.round_op(V, depth, op, r2, material=7)) and np.array_equal(preview, ctx.octree_extract())
                    all_ok &= ok
                    verdict = "matches numpy" if ok else "DIFFERS from numpy"
                print(f"  {name:6s} radius2 {r2:4d} (R {R:2d})  round {m * 1e3:8.2f} ms  step-wise conn 26 {step * 1e3:8.2f} ms  compact {base * 1e3:7.2f} ms  "
                      f"({m / step:5.2f}x step-wise)  {len(preview):>9d} voxels  {verdict}", flush=True)
                del buf
        del vbos
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
