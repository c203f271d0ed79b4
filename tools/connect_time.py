#!/usr/bin/env python3
"""Connected components on the GPU (tdt_octree_components / tdt_octree_edit_connected): wall-clock medians after warm-up on
configs 3 and 5 — labelling at 6- and 26-connectivity, a seed CLEAR of the largest component and a debris CLEAR (max 8 voxels),
against the same tree's tdt_octree_compact.  Labelling is timed as ONE call into buffers sized beforehand (labels and table,
or the table alone), and through Context.octree_components, which adds the walk that sizes the labels.  Every result is checked
against the numpy model (tests/connect_model.py).

    python tools/connect_time.py [--reps N] [--warmup N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import connect_model as cm  # noqa: E402
from test_gpu_region_edit import built_cells, padded  # noqa: E402
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
        orig = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
        ctx = rt.Context(0)
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        labels6, tab6 = cm.components(V, depth, 6, rt.MATCH_ANY)
        labels26, tab26 = cm.components(V, depth, 26, rt.MATCH_ANY)
        largest = V[tab6["first"][int(np.argmax(tab6["voxels"]))], :3]
        print(f"config {cfg}: depth {depth}, {len(V)} voxels, {len(orig) // 16} cells, {len(tab6)} components at 6, {len(tab26)} at 26")
        room = len(orig) // 16

        def reset():
            buf.sub_data(0, padded(orig, 64 * room))
            ctx.finish()

        buf = rt.VertexBufferObject(ctx, padded(orig, 64 * room))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)
        base, _ = timed(ctx.octree_compact, reset, a.reps, a.warmup)
        ok = np.array_equal(buf.read(np.uint32), padded(built_cells(ctx, V, depth), 64 * room))
        all_ok &= ok
        print(f"  {'compact':26s} median {base * 1e3:7.2f} ms  {'matches numpy' if ok else 'DIFFERS from numpy'}")
        L = rt.lib()
        for conn, want_l, want_t in ((6, labels6, tab6), (26, labels26, tab26)):
            labels = np.zeros(len(want_l), np.uint32)           # sized beforehand: one call labels once
            tab = np.zeros(len(want_t), rt.COMPONENT_DTYPE)
            nv, nc = rt.ctypes.c_size_t(0), rt.ctypes.c_size_t(0)
            got = {}

            def clear():                                        # not timed: the check below sees this call's output only
                labels[:] = 0
                tab[:] = 0
                got.clear()
                ctx.finish()

            def one_call(with_labels, conn=conn):
                ctx.check(L.tdt_octree_components(ctx.h, conn, 0, labels.ctypes.data if with_labels else None, len(labels), rt.ctypes.byref(nv),
                                                  tab.ctypes.data, len(tab), rt.ctypes.byref(nc)))

            def wrapper(conn=conn):
                got["r"] = ctx.octree_components(conn, rt.MATCH_ANY)

            for name, f, check in ((f"labels + table at {conn}", lambda: one_call(True),
                                    lambda: np.array_equal(labels, want_l) and tab.tobytes() == want_t.tobytes()),
                                   (f"table only at {conn}", lambda: one_call(False), lambda: tab.tobytes() == want_t.tobytes()),
                                   (f"octree_components at {conn}", wrapper,
                                    lambda: np.array_equal(got["r"][0], want_l) and got["r"][1].tobytes() == want_t.tobytes())):
                med, best = timed(f, clear, a.reps, a.warmup)
                ok = bool(check())
                all_ok &= ok
                print(f"  {name:26s} median {med * 1e3:7.2f} ms  min {best * 1e3:7.2f} ms  ({med / base:4.2f}x compact)  "
                      f"{'matches numpy' if ok else 'DIFFERS from numpy'}")
        for name, kw in (("seed CLEAR of the largest", dict(seeds=[largest])), ("debris CLEAR max 8", dict(min_voxels=1, max_voxels=8))):
            want_vox = cm.edit(V, depth, rt.REGION_CLEAR, **kw)
            built = built_cells(ctx, want_vox, depth)
            med, best = timed(lambda: ctx.octree_edit_connected(rt.REGION_CLEAR, **kw), reset, a.reps, a.warmup)
            ok = np.array_equal(buf.read(np.uint32), padded(built, 64 * room))
            all_ok &= ok
            print(f"  {name:26s} median {med * 1e3:7.2f} ms  min {best * 1e3:7.2f} ms  ({med / base:4.2f}x compact)  "
                  f"{len(want_vox):>8d} voxels -> {len(built) // 16:>7d} cells  {'matches numpy' if ok else 'DIFFERS from numpy'}")
        del buf, vbos
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
