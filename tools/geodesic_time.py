#!/usr/bin/env python3
"""Geodesic distance on the GPU (tdt_octree_extract_geodesic / tdt_octree_geodesic_field): host wall-clock medians after warm-up
on configs 2, 3 and 5 (depths 6, 8 and 9), from ONE seed — a voxel in the middle of the tree's list (SOLID) and the nearest empty
voxel above it (EMPTY) — for the steps {1,0,0}, {1,1,1} and {3,4,5}, without a cost limit and with max_cost = 48.  The phases are
told apart by the forms that stop early, each timed in turn with the others so that they see the same machine state:

    walk    tdt_octree_extract counting only: the tree walk every form starts with
    relax   the field over a one-voxel box minus the walk: bounding box, rasterise, medium, seed and the relaxation passes
    list    the list form minus that field: reach bits, count, scan, emit, sort, list and the copy to the host

Beside them the units that compute the unlimited reach sets without distances: tdt_octree_extract_connected from the same seed
(SOLID) and tdt_octree_extract_enclosed (EMPTY: the flood from the grid's faces; its complement is the reach from the faces, not
from the one seed, so it is the yardstick of a whole-grid flood, not the same set).  Every list is checked against the numpy
model (tests/geodesic_model.py) on trees up to --check-depth; deeper trees are reported as unchecked.

    python tools/geodesic_time.py [--reps N] [--warmup N] [--configs 2,3,5] [--check-depth 6]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import geodesic_model as gm  # noqa: E402
from test_gpu_region_edit import morton  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402

STEPS = (rt.STEPS_6, rt.STEPS_26, rt.CHAMFER_345)


def timed(fns, reps, warmup):
    """Medians of the functions, called in turn (every call synchronises)."""
    ts = [[] for _ in fns]
    for i in range(warmup + reps):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                t.append(time.perf_counter() - t0)
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--check-depth", type=int, default=6)
    a = ap.parse_args()
    all_ok = True
    for cfg in [int(c) for c in a.configs.split(",")]:
        scene = host.Scene.config(cfg)
        depth = scene.max_depth
        n = 1 << depth
        ctx = rt.Context(0)
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        keys = morton(V[:, :3])
        solid_seed = V[len(V) // 2, :3].astype(np.int64)
        up = solid_seed + np.arange(1, n)[:, None] * np.array([0, 0, 1])
        up = up[up[:, 2] < n]
        free = up[~np.isin(morton(up), keys)]
        empty_seed = free[0] if len(free) else None
        print(f"config {cfg}: depth {depth}, {len(V)} voxels, solid seed {solid_seed.tolist()}, empty seed {None if empty_seed is None else empty_seed.tolist()}",
              flush=True)
        walk, conn6, conn26, enc6, enc26 = timed([ctx._voxel_count, lambda: ctx.octree_extract_connected(seeds=[solid_seed], connectivity=6),
                                                  lambda: ctx.octree_extract_connected(seeds=[solid_seed], connectivity=26),
                                                  lambda: ctx.octree_extract_enclosed(6, material=0), lambda: ctx.octree_extract_enclosed(26, material=0)],
                                                 a.reps, a.warmup)
        print(f"  walk {walk * 1e3:7.2f} ms   extract_connected 6 / 26 {conn6 * 1e3:8.2f} / {conn26 * 1e3:8.2f} ms   "
              f"extract_enclosed 6 / 26 {enc6 * 1e3:8.2f} / {enc26 * 1e3:8.2f} ms (each counts, then fills: two floods)", flush=True)
        for medium, name, seed in ((rt.MEDIUM_SOLID, "SOLID", solid_seed), (rt.MEDIUM_EMPTY, "EMPTY", empty_seed)):
            if seed is None:
                continue
            for w in STEPS:
                for max_cost in (1 << 30, 48):
                    kw = dict(medium=medium, steps=w, max_cost=max_cost)
                    box = tuple(int(v) for v in seed)
                    g = rt.Context._geodesic(medium, w, max_cost, None, 0, [seed])
                    limit = "unlimited" if max_cost == 1 << 30 else f"max {max_cost:4d}"
                    try:
                        count = reach_count(ctx, g)
                    except rt.TdtError as e:                     # a reach set above 2^26 voxels has no list: the field form still runs
                        field, _ = timed([lambda: ctx.octree_geodesic_field([seed], box, box, **kw), ctx._voxel_count], a.reps, a.warmup)
                        print(f"  {name} {str(w):9s} {limit:9s}  relax {max(field - walk, 0) * 1e3:8.2f} ms  passes {ctx.geodesic_passes():4d}  no list: {e}",
                              flush=True)
                        continue

                    def list_once():                             # one relaxation: the buffer is sized by the count taken before
                        out = np.zeros((max(count, 1), 4), np.int32)
                        nv = ctypes.c_size_t(0)
                        ctx.check(rt.lib().tdt_octree_extract_geodesic(ctx.h, ctypes.byref(g[0]), g[1].ctypes.data, 1, None, 0, out.ctypes.data, len(out),
                                                                       ctypes.byref(nv)))
                        return out[: nv.value]

                    field, lst, _ = timed([lambda: ctx.octree_geodesic_field([seed], box, box, **kw), list_once, ctx._voxel_count], a.reps, a.warmup)
                    passes = ctx.geodesic_passes()
                    verdict = "unchecked"
                    if depth <= a.check_depth:
                        ok = np.array_equal(list_once(), gm.reach_list(V, depth, [seed], material=0, **kw))
                        all_ok &= ok
                        verdict = "matches numpy" if ok else "DIFFERS from numpy"
                    base = (conn6 if w == rt.STEPS_6 else conn26) if medium == rt.MEDIUM_SOLID else (enc6 if w == rt.STEPS_6 else enc26) / 2
                    print(f"  {name} {str(w):9s} {limit:9s}  relax {max(field - walk, 0) * 1e3:8.2f} ms  list {max(lst - field, 0) * 1e3:7.2f} ms  "
                          f"total {lst * 1e3:8.2f} ms  passes {passes:4d}  {count:>9d} voxels  ({lst / base:5.2f}x the yes/no unit)  {verdict}", flush=True)
        del vbos
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


def reach_count(ctx, g):
    """|R| from the count-only list call."""
    nv = ctypes.c_size_t(0)
    ctx.check(rt.lib().tdt_octree_extract_geodesic(ctx.h, ctypes.byref(g[0]), g[1].ctypes.data, 1, None, 0, None, 0, ctypes.byref(nv)))
    return int(nv.value)


if __name__ == "__main__":
    sys.exit(main())
