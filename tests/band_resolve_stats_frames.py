"""Child process of tests/test_gpu_band_resolve.py: renders every frame of band_resolve_cases.cases(DEPTH) with whatever library TDT_LIB
names (the statistics build) and prints, per frame, one JSON line with the pass statistics of its launch; the images go to
OUT_DIR/<case>.npy.
usage: band_resolve_stats_frames.py DEPTH OUT_DIR"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import band_resolve_cases as br
import test_gpu_five_waves as five
from tdt4230_project_raytracing_amd import rt

depth, out_dir = int(sys.argv[1]), sys.argv[2]
scene = five._scene(depth, "reference_corner")
for name, k, m in br.cases(depth):
    r = rt.Renderer(scene, br.camera(depth, k, m))
    try:
        r.ctx.stats()                                 # switches the collection on
        r.ctx.stats(reset=True)
        img = r.render()
        st = r.ctx.stats(reset=True)
        v = r.ctx.last_variant()
    finally:
        r.close()
    np.save(os.path.join(out_dir, name + ".npy"), img)
    keys = ("trav_pass", "trav_lanes", "fallback_pass", "fallback_lanes", "band_pass", "band_lanes", "resolved_lanes", "waves")
    print(json.dumps({"case": name} | {k_: st[k_] for k_ in keys} | {k_: v[k_] for k_ in ("block", "per_cu", "full")}), flush=True)
