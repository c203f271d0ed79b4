#!/usr/bin/env python3
"""Surface extraction on the GPU: host wall-clock medians after warm-up, every timed result checked against the numpy model
(tests/surface_model.py) as bytes.

  trees    configs 2, 3 and 5: tdt_octree_extract_surface into a buffer of the right size (one call: no count query), merge 0 and
           1, by_material 1, alternating call by call with tdt_octree_extract_morph(SHELL, 6, radius 1) of the same tree, also
           into a sized buffer.  That call does the same neighbour probe (one gallop_find per face neighbour) and one scan and
           gather, and no sorting: the difference is what the face sorts, the runs and the stacks cost.  Both walk the tree first.

    python tools/surface_time.py [--reps N] [--warmup N] [--configs 2,3,5] [--check-limit VOXELS]"""
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

import surface_model as sm  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402


def timed_pair(f, g, reps, warmup):
    """Medians of f and of g, called alternately, g first (every call synchronises)."""
    tf, tg = [], []
    for i in range(warmup + reps):
        for fn, ts in ((g, tg), (f, tf)):
            t = time.perf_counter()
            fn()
            if i >= warmup:
                ts.append(time.perf_counter() - t)
    return float(np.median(tf)), float(np.median(tg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--check-limit", type=int, default=1 << 24, help="voxels up to which the result is compared with the numpy model")
    a = ap.parse_args()
    L = rt.lib()
    all_ok = True
    for cfg in [int(c) for c in a.configs.split(",")]:
        scene = host.Scene.config(cfg)
        depth = scene.max_depth
        ctx = rt.Context(0)
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        shell = ctx.octree_extract_morph(rt.MORPH_SHELL, 1, 6)
        shell_out = np.zeros_like(shell)
        m = rt.Morph(rt.MORPH_SHELL, 6, 1, -1, 0, 0)
        ns = ctypes.c_size_t(0)

        def run_shell():
            ctx.check(L.tdt_octree_extract_morph(ctx.h, ctypes.byref(m), None, 0, shell_out.ctypes.data, len(shell_out), ctypes.byref(ns)))

        print(f"config {cfg}: depth {depth}, {len(V)} voxels, {len(shell)} surface voxels", flush=True)
        for merge in (0, 1):
            quads = ctx.octree_extract_surface(merge, 1)
            faces = int((quads[:, 5] * quads[:, 6]).sum())
            out = np.zeros_like(quads)
            opt = rt.Surface(merge, 1)
            nq = ctypes.c_size_t(0)

            def run_surface():
                ctx.check(L.tdt_octree_extract_surface(ctx.h, ctypes.byref(opt), None, 0, out.ctypes.data, len(out), ctypes.byref(nq)))

            t_surface, t_shell = timed_pair(run_surface, run_shell, a.reps, a.warmup)
            if len(V) <= a.check_limit:
                ok = out.tobytes() == sm.quads(V, depth, merge, 1).tobytes() and np.array_equal(shell_out, shell)
                all_ok &= ok
                verdict = "matches numpy" if ok else "DIFFERS from numpy"
            else:
                verdict = "not compared (above --check-limit)"
            print(f"  merge {merge}  median {t_surface * 1e3:8.2f} ms  shell extract {t_shell * 1e3:7.2f} ms  ({t_surface / t_shell:5.2f}x)  "
                  f"{faces:>9d} faces {faces / t_surface / 1e6:8.1f} M/s  {len(quads):>9d} quads {len(quads) / t_surface / 1e6:8.1f} M/s  {verdict}",
                  flush=True)
        del vbos
        ctx.close()
    print(f"reps {a.reps}, warm-up {a.warmup}; " + ("all checks pass" if all_ok else "SOME CHECKS FAILED"))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
