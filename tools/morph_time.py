#!/usr/bin/env python3
"""Voxel morphology on the GPU (tdt_octree_morph): host wall-clock medians after warm-up on configs 3 and 5 — ERODE, SHELL,
DILATE, OPEN and CLOSE at radius 1 and 4, connectivity 6 and 26 — each alternating, call by call, with tdt_octree_compact of the
same tree (the rebuild every edit pays; an operation this unit does not touch), so both see the same machine state.  Every timed
result is checked against the numpy model (tests/morph_model.py).  Per op and connectivity the per-step increment
(radius 4 - radius 1) / 3 is printed on its own line: further steps add list passes, no rebuild.

    python tools/morph_time.py [--reps N] [--warmup N] [--configs 3,5] [--radii 1,4]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import morph_model as mm  # noqa: E402
from test_gpu_region_edit import built_cells, padded  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402

OPS = (("ERODE", rt.MORPH_ERODE), ("SHELL", rt.MORPH_SHELL), ("DILATE", rt.MORPH_DILATE), ("OPEN", rt.MORPH_OPEN), ("CLOSE", rt.MORPH_CLOSE))


def timed_pair(f, g, reset, reps, warmup):
    """Medians of f and of g, called alternately, g first (reset() before each, not timed; every call synchronises): the buffer
    is left as the last call of f wrote it."""
    tf, tg = [], []
    for i in range(warmup + reps):
        for fn, ts in ((g, tg), (f, tf)):
            reset()
            t = time.perf_counter()
            fn()
            if i >= warmup:
                ts.append(time.perf_counter() - t)
    return float(np.median(tf)), float(np.median(tg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--radii", default="1,4")
    a = ap.parse_args()
    radii = [int(r) for r in a.radii.split(",")]
    all_ok = True
    for cfg in [int(c) for c in a.configs.split(",")]:
        scene = host.Scene.config(cfg)
        depth = scene.max_depth
        orig = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
        ctx = rt.Context(0)
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        print(f"config {cfg}: depth {depth}, {len(V)} voxels, {len(orig) // 16} cells", flush=True)
        cache = {}
        for conn in (6, 26):
            for name, op in OPS:
                med = {}
                for radius in radii:
                    want_vox = mm.morph(V, depth, op, radius, conn, cache=cache)
                    built = built_cells(ctx, want_vox, depth)
                    room = max(len(orig), len(built)) // 16 + 8
                    start = padded(orig, 64 * room)
                    buf = rt.VertexBufferObject(ctx, start)
                    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)

                    def reset():
                        buf.sub_data(0, start)
                        ctx.finish()

                    m, base = timed_pair(lambda: ctx.octree_morph(op, radius, conn), ctx.octree_compact, reset, a.reps, a.warmup)
                    ok = np.array_equal(buf.read(np.uint32), padded(built, 64 * room))
                    all_ok &= ok
                    med[radius] = m
                    print(f"  {name:6s} conn {conn:2d} radius {radius}  median {m * 1e3:8.2f} ms  compact {base * 1e3:7.2f} ms  ({m / base:5.2f}x compact)  "
                          f"{len(want_vox):>8d} voxels -> {len(built) // 16:>7d} cells  {'matches numpy' if ok else 'DIFFERS from numpy'}", flush=True)
                    del buf
                if len(radii) > 1 and radii[-1] > radii[0]:
                    step = (med[radii[-1]] - med[radii[0]]) / (radii[-1] - radii[0])
                    print(f"  {name:6s} conn {conn:2d} per further step  {step * 1e3:8.2f} ms", flush=True)
        del vbos
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
