"""Lanes in a band served from the whole-depth table (csrc/trace_device.hpp band_classify, band_resolve_x; the five-wave builds).

Frames: plane bundles with d_x = +0 (degenerate_cams.plane_bundle) whose plane lies m ulps beside a grid plane k of 2^D
(band_resolve_cases): every sample point of every primary ray has the one local coordinate lx = k / 2^D +- m ulp, inside the band of
k.  k is odd, 2 mod 4, and 2^(D - 1); m is 1, 3, 16, 60 and 120 on both sides.  Above k, and below an odd k, the lanes take a table
entry; below an even k the wave walks the levels as before.  Every frame, first and replay, equals the oracle bit for bit, on the
depth-5 and depth-6 trees of test_gpu_full_grid_corners; the statistics build (a process of its own, all frames of a depth in one)
says which path the lanes took.  tdt_selftest 19 checks the rule itself for every float of every band and every (y, z)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import band_resolve_cases as br
import band_resolve_model as model
import test_gpu_five_waves as five
import test_gpu_full_grid_corners as corners
import test_gpu_plane_table as planes
from tdt4230_project_raytracing_amd import build, rt

pytestmark = pytest.mark.gpu

POW2 = 1
LANES = br.W * br.H * br.SPP                    # primary rays of a frame: each has at least one step in the octree, in the band
CASES = [(d, name) for d in (5, 6) for name, _, _ in br.cases(d)]

_stats = {}


def _case(depth, name):
    return next((k, m) for n, k, m in br.cases(depth) if n == name)


def _stats_of(depth, tmp_path_factory):
    """The statistics build's frames of one depth: {case: (statistics, image)}, rendered once by one child process."""
    if depth not in _stats:
        assert os.path.exists(build.STATS_LIB), "build() makes the statistics library"
        out = str(tmp_path_factory.mktemp(f"band_resolve_d{depth}"))
        env = {**os.environ, "TDT_LIB": build.STATS_LIB}
        p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "band_resolve_stats_frames.py"), str(depth), out],
                           env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        rows = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
        _stats[depth] = {r["case"]: (r, np.load(os.path.join(out, r["case"] + ".npy"))) for r in rows}
    return _stats[depth]


@pytest.mark.parametrize("depth,name", CASES)
def test_frames_in_a_band_equal_the_oracle(oracle, tmp_path_factory, depth, name):
    k, m = _case(depth, name)
    side = br.side(depth, k, m)                                            # (asserts: in the band of k, off the plane, on the intended side)
    assert side == ("above" if m > 0 else ("odd_below" if k & 1 else "even_below"))
    scene, cam = five._scene(depth, "reference_corner"), br.camera(depth, k, m)
    ref = oracle.render(scene, cam, threads=4)
    r = rt.Renderer(scene, cam)
    try:
        first = r.render()
        v = r.ctx.last_variant()
        again = r.render()
    finally:
        r.close()
    assert planes._variant(v) == (POW2, depth, 1, 1, 0, 1) and five._geometry(v) == five.FIVE
    corners._same(first, ref, "first frame")
    corners._same(again, ref, "replay")
    st, img = _stats_of(depth, tmp_path_factory)[name]
    assert (st["block"], st["per_cu"]) == five.FIVE and st["full"] == 1
    print(f"depth {depth} {name}: band lanes {st['band_lanes']}, resolved {st['resolved_lanes']}, left to the walk {st['fallback_lanes']} in {st['fallback_pass']} of {st['trav_pass']} passes")
    if side == "even_below":
        assert st["fallback_lanes"] >= LANES, st
    else:
        assert st["resolved_lanes"] >= LANES, st
    corners._same(img, ref, "statistics build")


def _in_view(depth):
    """Finest-level (y, z) columns whose centre lies inside the bundle's fan: the eye at local (y, z) = (0.4, 0.7) looks along -z with
    a vertical field of 90 degrees."""
    side = 1 << depth
    c = (np.arange(side) + 0.5) / side
    y, z = np.meshgrid(c, c, indexing="ij")
    return (z < 0.7) & (np.abs(y - 0.4) < 0.7 - z)


@pytest.mark.parametrize("depth", [5, 6])
def test_both_outcomes_occur_among_the_frames_above_a_plane(depth):
    """Keeps the frames from passing vacuously (CPU, band_resolve_model): among the above-side frames there is a column in view where the
    walk ends in the cell of n - 2^j and that is not the cell of n, and one where it ends in the cell of n while n - 2^j names another."""
    cells = corners._tree(depth)
    yi, zi = np.nonzero(_in_view(depth))
    lower = upper = 0
    for _, k, m in br.cases(depth):
        if m < 0:
            continue
        lx = br.local_x(depth, k, m)
        j = int(model.trailing_zeros(k))
        want = model.walk(cells, depth, lx, yi, zi)
        at_n, at_low = model.plain(cells, depth, k, yi, zi)[:4], model.plain(cells, depth, k - (1 << j), yi, zi)[:4]
        is_n = np.logical_and.reduce([w == g for w, g in zip(want, at_n)])
        is_low = np.logical_and.reduce([w == g for w, g in zip(want, at_low)])
        assert (is_n | is_low).all()
        lower += int((is_low & ~is_n).sum())
        upper += int((is_n & ~is_low).sum())
    assert lower > 0 and upper > 0, (lower, upper)


@pytest.mark.parametrize("depth", [5, 6])
def test_selftest_19(depth):
    r = rt.Renderer(five._scene(depth, "reference_corner"), five._camera("reference_corner", 33, 33, 4))
    try:
        r.render()
        assert r.ctx.selftest(19) == 0
        counts = r.ctx.selftest_band_counts()
    finally:
        r.close()
    print(f"depth {depth}: {counts}")
    assert counts["to_n"] > 0 and counts["to_lower"] > 0 and counts["to_walk"] > 0, counts
