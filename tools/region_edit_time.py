#!/usr/bin/env python3
"""Region edits on the GPU (tdt_octree_edit_region): wall-clock medians after warm-up on configs 3 and 5 — spheres of radius 8
and 32 with SET and CLEAR, a whole-grid CLEAR, and the same tree's tdt_octree_compact as the baseline.  Every edit starts from
the scene's own bytes and its result is checked against the numpy-expected tree (tests/test_gpu_region_edit.py's model).

    python tools/region_edit_time.py [--reps N] [--warmup N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

from test_gpu_region_edit import built_cells, expected_region, padded  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402


def timed(f, reset, reps, warmup):
    """Median and min of `reps` calls after `warmup` (each call after reset(), which is not timed; every call synchronises)."""
    ts = []
    for i in range(warmup + reps):
        reset()
        t = time.perf_counter()
        f()
        if i >= warmup:
            ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    all_ok = True
    for cfg in (3, 5):
        scene = host.Scene.config(cfg)
        depth = scene.max_depth
        n = 1 << depth
        orig = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
        ctx = rt.Context(0)
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        c = V[len(V) // 2, :3].astype(int)
        cases = [("compact", None, None)]
        for r in (8, 32):
            for op in (rt.REGION_SET, rt.REGION_CLEAR):
                cases.append((f"sphere r={r} {'SET' if op == rt.REGION_SET else 'CLEAR'}", op, [rt.sphere(c, r)]))
        cases.append(("whole-grid CLEAR", rt.REGION_CLEAR, [rt.box((0, 0, 0), (n - 1, n - 1, n - 1))]))
        base = None
        print(f"config {cfg}: depth {depth}, {len(V)} voxels, {len(orig) // 16} cells")
        for name, op, regions in cases:
            want_vox = V if op is None else expected_region(V, op, regions, 5, depth)
            built = built_cells(ctx, want_vox, depth)
            room = max(len(orig) // 16, len(built) // 16)
            buf = rt.VertexBufferObject(ctx, padded(orig, 64 * room))
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)

            def reset():
                buf.sub_data(0, padded(orig, 64 * room))
                ctx.finish()

            f = ctx.octree_compact if op is None else (lambda: ctx.octree_edit_region(op, regions, 5))
            med, best = timed(f, reset, a.reps, a.warmup)
            ok = np.array_equal(buf.read(np.uint32), padded(built, 64 * room))
            all_ok &= ok
            if base is None:
                base = med
            print(f"  {name:22s} median {med * 1e3:7.2f} ms  min {best * 1e3:7.2f} ms  ({med / base:4.2f}x compact)  "
                  f"{len(want_vox):>8d} voxels -> {len(built) // 16:>7d} cells  {'matches numpy' if ok else 'DIFFERS from numpy'}")
            del buf
        del vbos
        ctx.close()
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
