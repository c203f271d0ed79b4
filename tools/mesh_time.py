#!/usr/bin/env python3
"""Triangle-mesh stamping on the GPU (tdt_octree_edit_triangles): host wall-clock medians after warm-up of a SET stamp of a
procedurally generated UV sphere and a torus, 10^3 .. 10^6 triangles, and of a few grid-spanning triangles, on the trees of
configs 2, 3 and 5 — each alternating, call by call, with tdt_octree_edit_voxels of the same resulting voxel list (the walk,
merge and rebuild every stamp pays; code this unit does not touch), so both see the same machine state.  The difference is the
rasteriser's cost.  Every timed result is checked against the numpy model (tests/mesh_model.py).  Printed per case:
milliseconds of both, the rasterise share of the whole stamp, and voxel tests per second counted as the voxels of the
triangles' grid-clipped bounding boxes (an upper bound of the level-2 tests: tiles the level-1 test rejects are never
enumerated).

    python tools/mesh_time.py [--reps N] [--warmup N] [--configs 2,3,5] [--counts 1000,10000,100000,1000000]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import mesh_model as mm  # noqa: E402
from test_gpu_region_edit import apply_op, built_cells, padded  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402


def timed_pair(f, g, reset, reps, warmup):
    """Medians of f and of g, called alternately, g first (reset() before each, not timed; every call synchronises)."""
    tf, tg = [], []
    for i in range(warmup + reps):
        for fn, ts in ((g, tg), (f, tf)):
            reset()
            t = time.perf_counter()
            fn()
            if i >= warmup:
                ts.append(time.perf_counter() - t)
    return float(np.median(tf)), float(np.median(tg))


def meshes(n, counts):
    """(name, float vertices in voxels, triangles) of every workload on a grid of side n."""
    c = n * 0.5
    for k in counts:
        s = max(int(round((k / 2) ** 0.5)), 3)
        yield f"sphere {2 * s * (s - 1):>8d}", *mm.uv_sphere((c, c, c), n * 0.42, s, s)
        yield f"torus  {2 * s * s:>8d}", *mm.torus((c, c, c), n * 0.3, n * 0.12, s, s)
    v = np.array([[0, 0, 0], [n, n / 2, n], [n / 2, n, n], [n, 0, 0], [0, n, n / 3], [0, n / 2, n], [0, 0, n], [n, n, n / 4], [n, n / 3, 0]], np.float32)
    yield "spanning        3", v, np.arange(9, dtype=np.uint32).reshape(3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--counts", default="1000,10000,100000,1000000")
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    all_ok = True
    for cfg in [int(c) for c in a.configs.split(",")]:
        scene = host.Scene.config(cfg)
        depth = scene.max_depth
        n = 1 << depth
        orig = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
        ctx = rt.Context(0)
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        print(f"config {cfg}: depth {depth}, {len(V)} voxels, {len(orig) // 16} cells", flush=True)
        for name, fv, tris in meshes(n, counts):
            q = host.mesh_quantize(fv)
            B = mm.voxelize_many(q, tris, depth, None, 5)
            tri = q.astype(np.int64)[tris.astype(np.int64)]
            lo = np.maximum(np.floor_divide(tri.min(1) - 1, mm.UNIT), 0)
            hi = np.minimum(np.floor_divide(tri.max(1), mm.UNIT), n - 1)
            box_voxels = int(np.maximum(hi - lo + 1, 0).prod(1).sum())
            ok = np.array_equal(ctx.voxelize_triangles(q, tris, depth, None, 5), B)
            want_vox = apply_op(V, rt.REGION_SET, B, 0)
            built = built_cells(ctx, want_vox, depth)
            room = max(len(orig), len(built)) // 16 + 8
            start = padded(orig, 64 * room)
            buf = rt.VertexBufferObject(ctx, start)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)

            def reset():
                buf.sub_data(0, start)
                ctx.finish()

            stamp, base = timed_pair(lambda: ctx.octree_edit_triangles(rt.REGION_SET, q, tris, None, 5),
                                     lambda: ctx.octree_edit_voxels(rt.REGION_SET, B), reset, a.reps, a.warmup)
            ok = ok and np.array_equal(buf.read(np.uint32), padded(built, 64 * room))
            all_ok &= ok
            raster = stamp - base
            rate = box_voxels / raster if raster > 0 else float("nan")
            print(f"  {name} triangles  stamp {stamp * 1e3:8.2f} ms  edit_voxels {base * 1e3:8.2f} ms  rasterise {raster * 1e3:8.2f} ms "
                  f"({100 * raster / stamp:5.1f} % of the stamp)  {len(B):>8d} voxels  {box_voxels:>10d} box voxels  {rate / 1e6:9.1f} M tests/s  "
                  f"{'matches numpy' if ok else 'DIFFERS from numpy'}", flush=True)
            del buf
        del vbos
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
