#!/usr/bin/env python3
"""Affine transforms of a selection on the GPU (tdt_octree_extract_transform / tdt_octree_transform): host wall-clock medians
after warm-up on configs 3 (depth 8) and 5 (depth 10).  The selection is the sphere of radius N / 4 about the centre of the
grid; it is moved by (5, -3, 2), quarter-turned about z, rotated by 30 degrees about (1, 1, 1) and doubled, all about the centre.
Per transform: the LIST form (one call into a buffer sized beforehand) and the EDIT form (REGION_SET), alternating call by call
with what the library offered for a paste before: tdt_octree_extract_region of the same selection into host memory followed by
tdt_octree_edit_voxels(REGION_SET) of that list — the host's own transform of the list left out, so the baseline is a lower
bound of the old way and, unlike the new one, is only correct for a translation or a lattice symmetry — and with
tdt_octree_compact (the rebuild every edit pays).  --wall adds what the brick cull keeps of a thin wall turned by 45 degrees
(bricks of the domain against bricks kept): the case a finer cull would have to win.

Every timed result is checked: against the numpy model (tests/xform_model.py) on trees up to --check-depth (the dense model
walks every voxel of the grid); on deeper trees every result voxel's source is recomputed and looked up in the selection
("sound": nothing wrong was produced), and for the bijections (move, turn) the forward image of the selection is compared too
("exact").

    python tools/xform_time.py [--reps N] [--warmup N] [--configs 3,5] [--check-depth 8] [--wall]"""
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

import xform_model as xm  # noqa: E402
from test_gpu_region_edit import apply_op, padded, sort_vox  # noqa: E402
from tdt4230_project_raytracing_amd import rt  # noqa: E402
from tdt4230_project_raytracing_amd import host  # noqa: E402


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


def forward(S, d=None, n=0):
    """The forward image of the list S under a move by d or one quarter turn about z through the centre of a grid of side n."""
    out = S.copy()
    if d is not None:
        out[:, :3] += np.array(d, np.int32)
    else:
        out[:, 0], out[:, 1] = n - 1 - S[:, 1], S[:, 0]
    return sort_vox(out[((out[:, :3] >= 0) & (out[:, :3] < n)).all(1)])


def check(V, S, depth, x, mask, got, kind, check_depth):
    n = 1 << depth
    if depth <= check_depth:
        return "matches numpy" if np.array_equal(got, xm.transform(V, depth, x, mask)) else "DIFFERS from numpy"
    s = xm.source_of(x, got[:, :3])
    lin = lambda p: (p[:, 0].astype(np.int64) * n + p[:, 1]) * n + p[:, 2]     # noqa: E731
    keys = lin(S[:, :3])
    order = np.argsort(keys)
    at = np.minimum(np.searchsorted(keys[order], lin(s)), len(keys) - 1)
    sound = ((s >= 0) & (s < n)).all() and np.array_equal(keys[order][at], lin(s)) and np.array_equal(S[order][at][:, 3], got[:, 3])
    if not sound:
        return "UNSOUND"
    if kind == "move":
        return "exact" if np.array_equal(got, forward(S, d=(5, -3, 2), n=n)) else "DIFFERS from the moved list"
    if kind == "turn":
        return "exact" if np.array_equal(got, forward(S, n=n)) else "DIFFERS from the turned list"
    return "sound (completeness unchecked at this depth)"


def list_call(ctx, x, arr, k, out):
    n = ctypes.c_size_t(0)
    ctx.check(rt.lib().tdt_octree_extract_transform(ctx.h, ctypes.byref(x), arr, k, out.ctypes.data, len(out), ctypes.byref(n)))
    return n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--check-depth", type=int, default=8)
    ap.add_argument("--wall", action="store_true")
    a = ap.parse_args()
    all_ok = True
    for cfg in [int(c) for c in a.configs.split(",")]:
        scene = host.Scene.config(cfg)
        depth = scene.max_depth
        n = 1 << depth
        orig = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
        ctx = rt.Context(0)
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        mask = [rt.sphere((n // 2,) * 3, n // 4)]
        arr, k = rt._touch_regions(mask)
        S = ctx.octree_extract_region(mask)
        print(f"config {cfg}: depth {depth}, {len(V)} voxels, {len(orig) // 16} cells; selection: sphere r {n // 4}, {len(S)} voxels", flush=True)
        c2, c = (n, n, n), (n / 2,) * 3
        cases = [("move", xm.translate((5, -3, 2))), ("turn", xm.quarter_turns(2, 1, c2)), ("rotate 30", xm.rotation((1, 1, 1), 30.0, c)),
                 ("x2", xm.scale((2,) * 3, (1,) * 3, c2))]
        for kind, x in cases:
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, vbos[0])
            xs = rt.Context._xform(x.fields())
            preview = ctx.octree_extract_transform(xs, mask)
            domain, kept = ctx.xform_bricks()
            room = len(orig) // 16 + 8
            while True:                                          # size the buffer for the largest result: a misfit reports its need
                start = padded(orig, 64 * room)
                buf = rt.VertexBufferObject(ctx, start)
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)
                try:
                    ctx.octree_transform(xs, rt.REGION_SET, mask)
                    break
                except rt.TdtError as e:
                    if not getattr(e, "n_cells", 0):
                        raise
                    room = e.n_cells + 8
            after = ctx.octree_extract()
            out, sel = np.zeros((len(preview), 4), np.int32), np.zeros((len(S), 4), np.int32)

            def reset():
                buf.sub_data(0, start)
                ctx.finish()

            def paste():
                m = ctypes.c_size_t(0)
                ctx.check(rt.lib().tdt_octree_extract_region(ctx.h, arr, k, sel.ctypes.data, len(sel), ctypes.byref(m)))
                ctx.octree_edit_voxels(rt.REGION_SET, sel)

            t_list, t_edit, t_paste, t_base = timed([lambda: list_call(ctx, xs, arr, k, out), lambda: ctx.octree_transform(xs, rt.REGION_SET, mask),
                                                     paste, ctx.octree_compact], reset, a.reps, a.warmup)
            verdict = check(V, S, depth, x, mask, preview, kind, a.check_depth)
            ok = (verdict in ("matches numpy", "exact") or verdict.startswith("sound")) and np.array_equal(out, preview)
            ok = ok and np.array_equal(after, apply_op(V, rt.REGION_SET, preview, None))
            all_ok &= ok
            print(f"  {kind:9s} list {t_list * 1e3:8.2f} ms  edit {t_edit * 1e3:8.2f} ms  extract_region + edit_voxels {t_paste * 1e3:8.2f} ms  "
                  f"compact {t_base * 1e3:7.2f} ms  {len(preview):>9d} voxels  bricks {domain} -> {kept}  {verdict if ok else 'FAILED: ' + verdict}", flush=True)
            del buf
        del vbos
        ctx.close()
    if a.wall:                                                   # what the bounding-box cull keeps of a thin wall turned by 45 degrees
        for depth in (8, 10):
            n = 1 << depth
            g = np.stack(np.meshgrid(np.arange(n // 4, 3 * n // 4), np.arange(n // 4, 3 * n // 4), indexing="ij"), -1).reshape(-1, 2)
            wall = np.concatenate([g[:, :1], np.full((len(g), 1), n // 2), g[:, 1:], np.full((len(g), 1), 5)], 1).astype(np.int32)
            ctx = rt.Context(0)
            vbo, _ = rt.octree_build_cells(ctx, sort_vox(wall), depth)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, vbo)
            ints = rt.VertexBufferObject(ctx, np.array([depth, 64, n], np.int32))
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
            xs = rt.Context._xform(xm.rotation((0, 0, 1), 45.0, (n / 2,) * 3).fields())
            preview = ctx.octree_extract_transform(xs)
            domain, kept = ctx.xform_bricks()
            out = np.zeros((len(preview), 4), np.int32)
            (t_list,) = timed([lambda: list_call(ctx, xs, None, 0, out)], ctx.finish, a.reps, a.warmup)
            print(f"wall depth {depth}: {len(wall)} voxels turned 45 degrees: list {t_list * 1e3:8.2f} ms  {len(preview)} voxels  bricks {domain} -> {kept} "
                  f"({512 * kept / max(len(preview), 1):.0f} candidates per result voxel)", flush=True)
            ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
