#!/usr/bin/env python3
"""Face tools on the GPU (tdt_octree_face_regions / tdt_octree_edit_faces): host wall-clock medians after warm-up on three trees —
a large flat wall (few huge regions), a terrain-like height field (terraces: regions of every size) and random noise (a tree of many
small regions).  Per tree, called alternately so that all see the same machine state:

    surface   tdt_octree_extract_surface(merge = 0), counting only (no array): the yardstick — the walk, the probe, the scan, the
              emit and the six sorts that the labelling shares with it, and nothing else
    label     tdt_octree_face_regions, counting only, with the hook stage's in-wave pre-merge of runs (the default)
    plain     the same with tdt_debug_faces_premerge(0): the A/B of stage 2
    pull      tdt_octree_edit_faces(FILL, one seed on the largest +z region, distance 8): label + seeds + columns + the region
              edit's walk, merge and rebuild

Printed: milliseconds of each, label / surface, plain / label, the faces and regions, and whether the two hooks returned the same
labels and table.  No ratio is asserted.

    python tools/faces_time.py [--reps N] [--warmup N] [--trees wall,terrain,noise]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tdt4230_project_raytracing_amd import rt  # noqa: E402


def wall(depth=9):
    """A slab 4 voxels thick across the whole grid."""
    n = 1 << depth
    x, y, z = np.meshgrid(np.arange(n), np.arange(n), np.arange(n // 2, n // 2 + 4), indexing="ij")
    return depth, np.stack([x.ravel(), y.ravel(), z.ravel(), np.full(x.size, 3)], 1).astype(np.int32)


def terrain(depth=8):
    """A height field of smooth hills quantised into terraces, solid below the surface down to 16 voxels under it."""
    n = 1 << depth
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    h = n / 2 + n / 6 * np.sin(x / 37.0) * np.cos(y / 23.0) + n / 10 * np.sin((x + 2 * y) / 61.0)
    h = (h // 3 * 3).astype(np.int64)
    cols = []
    for k in range(16):
        z = h - k
        cols.append(np.stack([x.ravel(), y.ravel(), z.ravel(), 1 + (z.ravel() // 16) % 5], 1))
    return depth, np.concatenate(cols).astype(np.int32)


def noise(depth=7):
    """Every other voxel at random: nearly every face is a region of its own."""
    n = 1 << depth
    rng = np.random.default_rng(1)
    p = np.argwhere(rng.random((n, n, n)) < 0.5)
    return depth, np.concatenate([p, rng.integers(1, 4, (len(p), 1))], 1).astype(np.int32)


def timed(fns, reset, reps, warmup):
    """Medians of the calls of fns, taken in turn (reset() before each, not timed; every call synchronises)."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trees", default="wall,terrain,noise")
    a = ap.parse_args()
    L = rt.lib()
    all_ok = True
    for name in a.trees.split(","):
        depth, vox = {"wall": wall, "terrain": terrain, "noise": noise}[name]()
        ctx = rt.Context(0)
        built, n_cells = rt.octree_build_cells(ctx, vox, depth)
        cells = built.read(np.uint32)
        room = n_cells + 8 * (1 << (2 * depth)) + 64                 # a pull by 8 adds at most 8 layers of single voxels
        start = np.zeros(16 * room, np.uint32)
        start[: len(cells)] = cells
        buf = rt.VertexBufferObject(ctx, start)
        ints = rt.VertexBufferObject(ctx, np.array([depth, 64, 1 << depth], np.int32))
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, buf)
        ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, ints)
        out = {}
        for premerge in (True, False):
            ctx.debug_faces_premerge(premerge)
            out[premerge] = ctx.octree_face_regions(4, rt.MATCH_MATERIAL, capacity=1 << 20)
        ctx.debug_faces_premerge(True)
        faces, labels, table = out[True]
        ok = np.array_equal(labels, out[False][1]) and table.tobytes() == out[False][2].tobytes() and np.array_equal(faces, out[False][0])
        ok = ok and np.array_equal(faces, ctx.octree_extract_surface(merge=False))
        up = table[table["face"] == 5]
        big = up[np.argmax(up["faces"])]
        q = faces[big["first"]]
        seed = np.array([[q[2], q[3], q[4] - 1, 5]], np.int32)        # the quad's origin is the lattice corner: the owner is one below
        surf = rt.Surface(0, 1)
        nq, nf, nr = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)

        def surface():
            ctx.check(L.tdt_octree_extract_surface(ctx.h, ctypes.byref(surf), None, 0, None, 0, ctypes.byref(nq)))

        def label(premerge):
            def run():
                ctx.check(L.tdt_debug_faces_premerge(ctx.h, premerge))
                ctx.check(L.tdt_octree_face_regions(ctx.h, 4, rt.MATCH_MATERIAL, None, 0, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nr)))
            return run

        def reset():
            buf.sub_data(0, start)
            ctx.finish()

        def pull():
            ctx.debug_faces_premerge(True)
            return ctx.octree_edit_faces(rt.REGION_FILL, seed, 8)

        t_surface, t_label, t_plain, t_pull = timed([surface, label(1), label(0), pull], reset, a.reps, a.warmup)
        ctx.debug_faces_premerge(True)
        reset()                                                      # the last pull changed the tree
        columns = len(ctx.octree_extract_faces(seed, 8)) if ok else 0
        ok = ok and nq.value == nf.value == len(faces) and nr.value == len(table) and 0 < columns <= 8 * int(big["faces"])
        all_ok &= ok
        print(f"{name:8s} depth {depth:2d}  {len(vox):>8d} voxels  {len(faces):>8d} faces  {len(table):>8d} regions  largest +z {int(big['faces']):>7d}  "
              f"surface {t_surface * 1e3:8.2f} ms  label {t_label * 1e3:8.2f} ms ({t_label / t_surface:4.2f}x)  plain hook {t_plain * 1e3:8.2f} ms "
              f"({t_plain / t_label:4.2f}x of label)  pull 8 {t_pull * 1e3:8.2f} ms  {'hooks agree' if ok else 'CHECK FAILED'}", flush=True)
        del buf, ints, built
        ctx.close()
    print("all checks pass" if all_ok else "SOME CHECKS FAILED")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
