#!/usr/bin/env python3
"""Stroke brushes on the GPU (tdt_octree_edit_stroke): host wall-clock medians after warm-up of a SET stroke of a few lengths and
radii on the trees of configs 2, 3 and 5 — each alternating, call by call, with the same path applied the way it had to be
before: ONE tdt_octree_edit_region call whose shapes are dabs (spheres, or cubes for the cube nib), one per voxel step along the
path — so both see the same machine state.  The two do not leave the same tree (dabs are the stroke sampled at lattice steps;
the stroke is the exact sweep), so each is checked on its own: the stroke's voxel list against the numpy model
(tests/stroke_model.py), the tree it leaves against the builder's tree of SET(V, that list).  Printed per case: milliseconds of
both, the covered voxels, the candidate voxels each enumerates (the stroke: 512 per tile of the segments' clipped boxes, an upper
bound, since culled tiles are never walked; the dabs: the voxels of their clipped boxes, which the region edit refuses above
2^26), and whether the checks hold.  No ratio is asserted.

    python tools/stroke_time.py [--reps N] [--warmup N] [--configs 2,3,5] [--radii 1,4,16]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import stroke_model as sm  # noqa: E402
from test_gpu_region_edit import apply_op, built_cells, padded  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402


def timed_pair(f, g, reset, reps, warmup):
    """Medians of f and of g, called alternately, g first (reset() before each, not timed; every call synchronises); g None: f alone."""
    tf, tg = [], []
    for i in range(warmup + reps):
        for fn, ts in ((g, tg), (f, tf)):
            if fn is None:
                continue
            reset()
            t = time.perf_counter()
            fn()
            if i >= warmup:
                ts.append(time.perf_counter() - t)
    return float(np.median(tf)), (float(np.median(tg)) if tg else float("nan"))


def paths(n):
    """(name, points) of every path on a grid of side n: a short straight drag, the body diagonal, and a zigzag of 16 legs."""
    q = n // 4
    yield "short", np.array([[q, q, q], [2 * q, q + q // 2, q + q // 3]], np.int32)
    yield "diagonal", np.array([[0, 0, 0], [n - 1, n - 1, n - 1]], np.int32)
    zig = [[(n - 1) * (i & 1), (n - 1) * i // 16, (n - 1) * ((i >> 1) & 1)] for i in range(17)]
    yield "zigzag", np.array(zig, np.int32)


def steps_of(points):
    """The lattice points of a polyline at unit Chebyshev steps: where a dab per voxel step goes."""
    out = [points[:1].astype(np.int64)]
    for a, b in zip(points[:-1].astype(np.int64), points[1:].astype(np.int64)):
        k = int(np.abs(b - a).max())
        i = np.arange(1, k + 1)[:, None]
        out.append(a + (2 * i * (b - a) + k) // (2 * k))          # rounded to the nearest lattice point
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--radii", default="1,4,16")
    a = ap.parse_args()
    radii = [int(c) for c in a.radii.split(",")]
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
        for name, pts in paths(n):
            dabs = steps_of(pts)
            for shape, nib in ((rt.SHAPE_SPHERE, "sphere"), (rt.SHAPE_BOX, "box")):
                for r in radii:
                    if shape == rt.SHAPE_BOX and r != radii[len(radii) // 2]:
                        continue                                       # the cube nib at the middle radius only
                    B = sm.voxelize(pts, r, depth, material=5, shape=shape)
                    ok = np.array_equal(ctx.voxelize_stroke(pts, r, depth, material=5, shape=shape), B)
                    built = built_cells(ctx, apply_op(V, rt.REGION_SET, B, 0), depth)
                    if shape == rt.SHAPE_SPHERE:
                        regions = [rt.sphere(tuple(int(c) for c in p), r) for p in dabs]
                    else:
                        regions = [rt.box(tuple(int(c) - r for c in p), tuple(int(c) + r for c in p)) for p in dabs]
                    lo, hi = np.maximum(dabs - r, 0), np.minimum(dabs + r, n - 1)
                    dab_lanes = int(np.maximum(hi - lo + 1, 0).prod(1).sum())
                    tiles = sum(sm.tile_candidates(p, q, r, depth) for p, q in zip(pts[:-1], pts[1:]))
                    room = max(len(orig), len(built)) // 16 + 4 * len(B) // 7 + 64      # the dabs' tree is another one: leave it room
                    start = padded(orig, 64 * room)
                    buf = rt.VertexBufferObject(ctx, start)
                    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)

                    def reset():
                        buf.sub_data(0, start)
                        ctx.finish()

                    old = (lambda: ctx.octree_edit_region(rt.REGION_SET, regions, 5)) if dab_lanes <= rt.REGION_BRUSH_CAP else None
                    new, base = timed_pair(lambda: ctx.octree_edit_stroke(rt.REGION_SET, pts, r, material=5, shape=shape), old, reset,
                                           a.reps, a.warmup)
                    ok = ok and np.array_equal(buf.read(np.uint32), padded(built, 64 * room))
                    all_ok &= ok
                    was = f"{base * 1e3:9.2f} ms" if old else "over the 2^26 cap"
                    print(f"  {name:8s} {nib:6s} r {r:3d}  segments {len(pts) - 1:3d}  stroke {new * 1e3:8.2f} ms  {len(dabs):5d} dabs {was}  "
                          f"{len(B):>9d} voxels  stroke candidates {512 * tiles:>10d}  dab candidates {dab_lanes:>11d}  "
                          f"{'matches numpy' if ok else 'DIFFERS from numpy'}", flush=True)
                    del buf
        del vbos
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
