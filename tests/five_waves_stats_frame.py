"""Child process of test_gpu_five_waves.test_rays_that_walk_global_memory: renders that test's frame with whatever library TDT_LIB
names (the statistics build) and prints the pass statistics of the launch as one JSON line; the image goes to the given .npy path.
usage: five_waves_stats_frame.py DEPTH OUT.npy"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import test_gpu_five_waves as five
from tdt4230_project_raytracing_amd import rt

depth, out = int(sys.argv[1]), sys.argv[2]
r = rt.Renderer(five._scene(depth, "reference_corner"), five._plane_bundle(depth))
try:
    r.ctx.stats()                                     # switches the collection on
    r.ctx.stats(reset=True)
    img = r.render()
    st = r.ctx.stats(reset=True)
    v = r.ctx.last_variant()
finally:
    r.close()
np.save(out, img)
print(json.dumps({k: st[k] for k in ("trav_pass", "trav_lanes", "fallback_pass", "fallback_lanes", "waves")} | {k: v[k] for k in ("block", "per_cu", "full")}))
