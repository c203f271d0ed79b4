#!/usr/bin/env python3
"""Enclosed-space fill on the GPU: host wall-clock medians after warm-up, every timed result checked against the numpy model
(tests/fill_model.py, its sweep form: the grids are 256^3 and 512^3).

  trees    configs 2, 3 and 5, hollowed first with MORPH_SHELL (radius 1, 26-neighbourhood) so that there is something to fill:
           tdt_octree_fill_enclosed alternating, call by call, with tdt_octree_compact of the same tree (the yardstick of whole-tree
           edits: both walk the tree and rebuild it once), and the number of flood passes the fill queued.
  meshes   the UV spheres of tools/mesh_time.py on the same trees: tdt_octree_edit_triangles_solid (SET) alternating with
           tdt_octree_edit_triangles of the same mesh, and the solid's flood passes.

    python tools/fill_time.py [--reps N] [--warmup N] [--configs 2,3,5] [--mesh-configs 2,3] [--counts 1000,100000]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import fill_model as fm  # noqa: E402
import mesh_model as mm  # noqa: E402
from test_gpu_region_edit import apply_op, built_cells, padded  # noqa: E402
from tdt4230_project_raytracing_amd import host, rt  # noqa: E402


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


def bound(ctx, start):
    buf = rt.VertexBufferObject(ctx, start)
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)

    def reset():
        buf.sub_data(0, start)
        ctx.finish()

    return buf, reset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--mesh-configs", default="2,3")           # (a solid sphere at depth 9 is 4 x 10^7 voxels: the model's minutes)
    ap.add_argument("--counts", default="1000,100000")
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
        S = ctx.octree_extract_morph(rt.MORPH_SHELL, 1, 26)      # tight under 26 as well: both connectivities have cavities to fill
        hollow = built_cells(ctx, S, depth)
        print(f"config {cfg}: depth {depth}, {len(V)} voxels, {len(orig) // 16} cells; hollowed: {len(S)} voxels, {len(hollow) // 16} cells", flush=True)
        for conn in (6, 26):
            want_vox = fm.filled(S, depth, conn, fast=True)
            built = built_cells(ctx, want_vox, depth)
            room = max(len(hollow), len(built)) // 16 + 8
            buf, reset = bound(ctx, padded(hollow, 64 * room))
            fill, base = timed_pair(lambda: ctx.octree_fill_enclosed(conn), ctx.octree_compact, reset, a.reps, a.warmup)
            ok = np.array_equal(buf.read(np.uint32), padded(built, 64 * room))
            all_ok &= ok
            print(f"  fill conn {conn:2d}  median {fill * 1e3:8.2f} ms  compact {base * 1e3:7.2f} ms  ({fill / base:5.2f}x compact)  "
                  f"{ctx.fill_passes():>4d} flood passes  {len(want_vox) - len(S):>8d} voxels filled -> {len(built) // 16:>7d} cells  "
                  f"{'matches numpy' if ok else 'DIFFERS from numpy'}", flush=True)
            del buf
        c = n * 0.5
        for k in counts if str(cfg) in a.mesh_configs.split(",") else []:
            s = max(int(round((k / 2) ** 0.5)), 3)
            fv, tris = mm.uv_sphere((c, c, c), n * 0.42, s, s)
            q = host.mesh_quantize(fv)
            surface = mm.voxelize_many(q, tris, depth, None, 5)
            solid = fm.filled(surface, depth, 6, fast=True)
            built = built_cells(ctx, apply_op(V, rt.REGION_SET, solid, 0), depth)
            shell = built_cells(ctx, apply_op(V, rt.REGION_SET, surface, 0), depth)      # the surface stamp's tree: a shell has more cells
            room = max(len(orig), len(built), len(shell)) // 16 + 8
            buf, reset = bound(ctx, padded(orig, 64 * room))
            stamp, base = timed_pair(lambda: ctx.octree_edit_triangles_solid(rt.REGION_SET, q, tris, None, 5),
                                     lambda: ctx.octree_edit_triangles(rt.REGION_SET, q, tris, None, 5), reset, a.reps, a.warmup)
            ok = np.array_equal(buf.read(np.uint32), padded(built, 64 * room))
            all_ok &= ok
            print(f"  sphere {2 * s * (s - 1):>8d} triangles  solid stamp {stamp * 1e3:8.2f} ms  surface stamp {base * 1e3:8.2f} ms  "
                  f"({stamp / base:5.2f}x)  {ctx.fill_passes():>4d} flood passes  {len(surface):>8d} surface + {len(solid) - len(surface):>9d} "
                  f"inside voxels  {'matches numpy' if ok else 'DIFFERS from numpy'}", flush=True)
            del buf
        del vbos
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
