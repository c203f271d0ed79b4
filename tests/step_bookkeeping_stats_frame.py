"""Child process of test_gpu_step_bookkeeping.test_statistics_build_counts_the_same_passes: renders that test's 8 x 8 frame with
whatever library TDT_LIB names (the statistics build; TDT_PIXEL_LOG=1 and, for the control, TDT_FOUR_WAVES=1 come with the
environment) and prints the pass statistics of the launch as one JSON line.  The .npz gets the image, the cost every pixel recorded
in that launch and, from an instrumented launch of the same frame, every pixel's traversal steps and events (all by queue slot).
usage: step_bookkeeping_stats_frame.py DEPTH OUT.npz"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import test_gpu_five_waves as five
from tdt4230_project_raytracing_amd import rt

depth, out = int(sys.argv[1]), sys.argv[2]
W = H = 8
r = rt.Renderer(five._scene(depth, "reference_corner"), five._camera("reference_corner", W, H, 4))
try:
    r.ctx.stats()                                     # switches the collection on
    r.ctx.stats(reset=True)
    img = r.render()
    st = r.ctx.stats(reset=True)
    v = r.ctx.last_variant()
    slots = r.shader.owned_tiles(W + 1, H + 1)[0] * 1024
    cost = r.shader.debug_pixel_log(slots)[:, 0].copy()
    r.shader.dispatch_counted(W + 1, H + 1)
    log = r.shader.debug_pixel_log(slots)
finally:
    r.close()
np.savez(out, image=img, cost=cost, steps=log[:, 0], events=log[:, 1])
keys = ("trav_pass", "trav_lanes", "inside_lanes", "event_pass", "event_lanes", "hit_pass", "hit_lanes", "end_pass", "end_lanes", "newray_lanes", "waves")
print(json.dumps({k: st[k] for k in keys} | {k: v[k] for k in ("block", "per_cu", "full")}))
