#!/usr/bin/env python3
"""Voxel extraction and compaction on the GPU (tdt_octree_census / _extract / _compact): times on the synthetic scenes and after
an edit session, each checked against the host builder's tree."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
from octree_util import distinct_deltas, edit_setup as setup, written_node
from tdt4230_project_raytracing_amd import host, rt


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = f(); ts.append(time.perf_counter() - t)
    return min(ts), out


def report(name, r, want, n_want):
    ctx = r.ctx
    t_census, census = best(ctx.octree_census)
    t_extract, vox = best(ctx.octree_extract)
    cells_before = r.vbos[0].read(np.uint32)
    t = time.perf_counter(); n = ctx.octree_compact(); t_compact = time.perf_counter() - t
    got = r.vbos[0].read(np.uint32)
    ok = n == n_want and np.array_equal(got[: 16 * n], want) and not got[16 * n:].any()
    t2, _ = best(ctx.octree_compact)                         # again, on the canonical tree
    print(f"{name}: {census['voxels']} voxels, {census['reachable_cells']} cells reached of {census['buffer_cells']} -> {n} cells; "
          f"census {t_census * 1e3:.2f} ms, extract {t_extract * 1e3:.2f} ms ({vox.nbytes / t_extract / 1e9:.1f} GB/s to the host), "
          f"compact {t_compact * 1e3:.2f} ms (canonical input {t2 * 1e3:.2f} ms); "
          f"{'identical to the host builder' if ok else 'DIFFERS from the host builder'}; {np.count_nonzero(cells_before != got)} words rewritten")


for cfg in (2, 3, 5):
    scene = host.Scene.config(cfg)
    want = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    r = rt.Renderer(scene, host.camera_reference_pose(64, 64, 1, 2))
    r.ctx.octree_census(); r.ctx.octree_compact()                   # warm the code objects
    report(f"config {cfg} ({scene.max_depth} levels)", r, want, scene.counts["cells"])
    r.close()

# an edit session on config 3: 32768 places, then their removals (the host builder's tree of config 3 is what must come back)
scene = host.Scene.config(3)
used, depth = scene.counts["cells"], scene.max_depth
want = np.ascontiguousarray(scene.blobs[0]).view(np.uint32).copy()
n = 32768
scene.blobs[0] = np.concatenate([want, np.zeros(16 * (n * depth + 8), np.uint32)])
d = distinct_deltas(np.random.default_rng(3), 2 * n, depth, scene.blobs[0])
d = d[[scene.blobs[0][2 * written_node(scene.blobs[0], p[:3], depth) + 1] == 0 for p in d]][:n]   # free blocks: removal undoes
place, remove = d.copy(), d.copy()
place[:, 3], place[:, 4] = 2.0, 1.0
remove[:, 3], remove[:, 4] = 0.0, 0.0
r, upd, counter = setup(scene, used, place)
upd.dispatch_compute(len(d), 1, 1)
r.vbos[5] = rt.VertexBufferObject(r.ctx, remove)
r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, r.vbos[5])
upd.dispatch_compute(len(d), 1, 1)
r.ctx.finish()
print(f"edit session: {len(d)} places + {len(d)} removes on config 3, counter {used} -> {int(counter.read(np.uint32)[0])}")
report("config 3 after the session", r, want, used)
r.close()
