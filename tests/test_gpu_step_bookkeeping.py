"""The traversal step's control bookkeeping in the scene-specialised builds (csrc/tdt_rt.hip trace_kernel, kMaskStep): a traversal
pass neither writes nor compares the lane state — who still traverses is mask algebra on the step's own compares and ONE compare
of the hit's word —, the hit records the slab test alone (whether the record is the root's or the leaf call site's is asked of the
iteration count in the event pass), and the iterations are counted down from max_iter against zero, once per step in the octree.

What moved is pinned here bit for bit against the oracle, once per build family: the whole-depth builds of depth 5 and 6 at
256 x 5 and, under TDT_FOUR_WAVES=1, at 1024 x 1, one brick build (depth 7) and one table-form build (depth 6).  Frames are at most
96 x 64 at 4 spp.  Every premise a case claims (hits in iteration 0, no hit in iteration 0, leaves found exactly at the iteration
limit, slab tests that fail at a leaf) is checked on the CPU with the oracle alone before the GPU is touched."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import degenerate_cams as dc
import test_gpu_build_matrix as bm
import test_gpu_degenerate_rays as dr
import test_gpu_five_waves as five
import test_gpu_raycast as rc
import tree_model
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, BOUNCE = 96, 64, 4, 4
FIVE, FOUR = (256, 5), (1024, 1)
# family: (row of test_gpu_build_matrix.ROWS, launch geometry, environment)
FAMILIES = {
    "full-d5": ((bm.POW2, 5, 1, 1, 0), FIVE, {}),
    "full-d6": ((bm.POW2, 6, 1, 1, 0), FIVE, {}),
    "full-d5-four": ((bm.POW2, 5, 1, 1, 0), FOUR, {"TDT_FOUR_WAVES": "1"}),
    "full-d6-four": ((bm.POW2, 6, 1, 1, 0), FOUR, {"TDT_FOUR_WAVES": "1"}),
    "brick-d7": ((bm.POW2, 7, 0, 0, 1), FOUR, {}),
    "table-d6": ((bm.TABLE, 6, 1, 0, 0), FOUR, {}),
}
ROOT_SHARE = 0.05                             # "many primary rays": a twentieth of the pixels show a hit of iteration 0

_cases, _refs = {}, {}


def _look(origin, view, w=W, h=H, spp=SPP, bounce=BOUNCE, fov=90.0):
    """test_gpu_build_matrix._camera for any image size, sample and bounce count."""
    d = np.asarray(view, np.float64)
    d = (d / np.linalg.norm(d)).astype(F)
    right = np.cross(d, np.array([0, 1, 0], F)).astype(F)
    right = (right / F(np.linalg.norm(right))).astype(F)
    up = np.cross(right, d).astype(F)
    vh = F(2.0 * np.tan(np.radians(fov) / 2.0))
    hor, ver = right * (F(F(w) / F(h)) * vh), up * vh
    o = np.asarray(origin, F)
    llc = o - hor * F(0.5) - ver * F(0.5) + d
    u = host.CameraUniforms()
    u.image_width, u.image_height, u.samples_per_pixel, u.max_bounce = w, h, spp, bounce
    for name, v in (("horizontal", hor), ("vertical", ver), ("lower_left_corner", llc), ("origin", o)):
        getattr(u, name)[:] = [float(x) for x in v.astype(F)]
    return u


def _env(monkeypatch, family):
    row, _, env = FAMILIES[family]
    for name in bm.row_switches(row):
        monkeypatch.setenv(name, "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _placed(family, unit=1):
    """(scene, corner, edge of the detail block) of the family's row, placed as test_gpu_build_matrix places it."""
    key = (FAMILIES[family][0], unit)
    if key not in _cases:
        scene, block = bm._scene(key[0])
        corner = (bm.UNIT_CORNER if unit else bm.ZERO_CORNERS[0]).astype(F)
        _cases[key] = (tree_model.with_corner(scene, corner), corner, F(block))
    return _cases[key]


def _inside(corner, block, **kw):
    """The reference pose scaled into the detail block, looking along -z (test_gpu_build_matrix._cameras)."""
    return _look(corner + block * np.array([0.5, 0.4, 0.7], F), (0.0, 0.0, -1.0), **kw)


def _outside(corner, block, **kw):
    """Just beyond the min corner, looking at the block's middle: every ray that meets the octree enters through a min face."""
    eye = np.array([-0.05, -0.05, -0.05], F)
    return _look(corner + block * eye, np.array([0.5, 0.4, 0.5]) - eye.astype(np.float64), fov=45.0, **kw)


def _front(corner, block, **kw):
    """In front of the min z face, looking along +z: the face's cells are what the rays meet first (hits in iteration 0)."""
    return _look(corner + block * np.array([0.5, 0.3, -0.3], F), (0.0, 0.0, 1.0), fov=60.0, **kw)


def _oracle(oracle, scene, cam):
    key = (id(scene), dc.camera_bits(cam).tobytes(), cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_bounce)
    if key not in _refs:
        ref = oracle.render(scene, cam, threads=8)
        ref.setflags(write=False)
        _refs[key] = (scene, ref)                                         # (the scene is kept: its id is part of the key)
    return _refs[key][1]


def _check(family, scene, cam, ref, what, unit=1):
    """First frame and cost-ordered replay of `cam` on the family's build, against `ref`."""
    row, geometry, _ = FAMILIES[family]
    first, again, v1, v2 = dr._render_twice(scene, cam)
    for v in (v1, v2):
        assert (v["form"], v["depth"], v["resident"], v["full"], v["brick"], v["unit"]) == row + (unit,), what
        assert (v["block"], v["per_cu"]) == geometry, what
    dr._assert_frame(first, ref, f"{what}, first frame")
    dr._assert_frame(again, ref, f"{what}, replay")


def _iteration_0_share(oracle, scene, cam):
    """Share of the pixels in which a leaf found in iteration 0 shows: under max_iter = 1 no other iteration runs."""
    one = bm._with_ints(scene, max_iter=1)
    return dc.differ(oracle.render(one, cam, threads=8), oracle.render(dc.empty_tree(one), cam, threads=8))


# ---- the record's call site ------------------------------------------------------------------------------------------------
def _five_cameras(placement):
    """`later`: test_gpu_five_waves' eye inside the octree.  `root`: an eye in front of the min x face of the level-1 LEAF octant
    (0, 1, 0) of test_gpu_full_grid_corners' trees, looking along +x: every primary ray enters the octree into that leaf."""
    corner, scale, _ = five.PLACEMENTS[placement]
    eye = np.array(corner, F) + np.array([-0.25, 0.75, 0.25], F) * F(scale)
    return {"later": five._camera(placement, W, H, SPP), "root": _look(eye, (1.0, 0.0, 0.0), fov=60.0)}


@pytest.mark.parametrize("site", ["root", "later"])
@pytest.mark.parametrize("placement", list(five.PLACEMENTS))
@pytest.mark.parametrize("family", [f for f in FAMILIES if f.startswith("full")])
def test_call_site_whole_depth(oracle, monkeypatch, family, placement, site):
    _env(monkeypatch, family)
    row, geometry, _ = FAMILIES[family]
    depth = row[1]
    scene, cam = five._scene(depth, placement), _five_cameras(placement)[site]
    ref = oracle.render(scene, cam, threads=8)
    assert dc.differ(ref, oracle.render(dc.empty_tree(scene), cam, threads=8)) >= 0.1, "the tree is not in view"
    share = _iteration_0_share(oracle, scene, cam)
    print(f"{family} {placement} {site}: iteration-0 hits show in {share:.3f} of the pixels")
    assert share >= ROOT_SHARE if site == "root" else share == 0.0, share
    first, again, v1, v2 = dr._render_twice(scene, cam)
    for v in (v1, v2):
        assert five.planes._variant(v) == (bm.POW2, depth, 1, 1, 0, five.PLACEMENTS[placement][2]) and five._geometry(v) == geometry
    dr._assert_frame(first, ref, "first frame")
    dr._assert_frame(again, ref, "replay")


@pytest.mark.parametrize("site", ["root", "later"])
@pytest.mark.parametrize("unit", [1, 0], ids=["unit", "mul"])
@pytest.mark.parametrize("family", ["brick-d7", "table-d6"])
def test_call_site_brick_and_table(oracle, monkeypatch, family, unit, site):
    _env(monkeypatch, family)
    scene, corner, block = _placed(family, unit)
    cam = (_front if site == "root" else _inside)(corner, block)
    ref = _oracle(oracle, scene, cam)
    assert dc.differ(ref, oracle.render(dc.empty_tree(scene), cam, threads=8)) >= 0.1, "the tree is not in view"
    share = _iteration_0_share(oracle, scene, cam)
    print(f"{family} unit={unit} {site}: iteration-0 hits show in {share:.3f} of the pixels")
    assert share >= ROOT_SHARE if site == "root" else share == 0.0, share
    _check(family, scene, cam, ref, site, unit)


# ---- a slab test that fails at a leaf ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_failed_slab_test_at_a_leaf(oracle, monkeypatch, family):
    """test_gpu_degenerate_rays' bundles: rays lying in a face plane of finest-level cells, whose slab operands at those leaves are
    NaN — the slab test fails at the leaf and the hit uses the record that is already there.  As frames, and the primary rays of
    the first bundle through pick and raycast."""
    _env(monkeypatch, family)
    row = FAMILIES[family][0]
    for name, scene, cam0, axis in dr._bundles(row, 1, bm.ROWS.index(row)):
        cam = dc.camera_from_bits(dc.camera_bits(cam0), W, H, SPP, BOUNCE)
        ref, st, share = dc.premises(oracle, scene, cam, axis, "nan")
        print(f"{family} {name}: nan_slab_tests {st['nan_slab_tests']} view share {share:.3f}")
        _check(family, scene, cam, ref, f"{name} bundle")
    name, scene, cam0, axis = dr._bundles(row, 1, bm.ROWS.index(row))[0]
    lamb, alb = rc._lambertian(scene)
    cam = dc.camera_from_bits(dc.camera_bits(cam0), dr.QW, dr.QH, SPP, 1)
    assert oracle.render(lamb, cam, threads=8, want_stats=True)[1]["nan_slab_tests"] >= dc.NAN_TESTS
    r = rt.Renderer(lamb, cam)
    try:
        hits, rays = r.pick(dr._XY, sample=0, return_rays=True)
        assert r.ctx.raycast(rays).tobytes() == hits.tobytes()
        n_hit, n_leaf = rc._assert_first_hit(oracle, lamb, alb, cam, hits, rays, 0, dr.QW, dr.QH)
    finally:
        r.close()
    assert n_leaf > 0, (n_hit, n_leaf)


# ---- the iteration limit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 2, 3, 7, None])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_iteration_limit(oracle, monkeypatch, family, max_iter):
    """max_iter set the way test_gpu_parity sets it (the second of the octree's ints).  The outside camera's rays find leaves from
    iteration 0 on; the frames under max_iter = m and m + 1 differ exactly where a leaf is found in iteration m — allowed under the
    second, one step too late under the first — so both sides of the limit are in the frame."""
    _env(monkeypatch, family)
    scene, corner, block = _placed(family)
    cam = _outside(corner, block)
    limited = scene if max_iter is None else bm._with_ints(scene, max_iter=max_iter)
    ref = oracle.render(limited, cam, threads=8)
    if max_iter is not None:
        beyond = dc.differ(ref, oracle.render(bm._with_ints(scene, max_iter=max_iter + 1), cam, threads=8))
        print(f"{family} max_iter {max_iter}: {beyond:.3f} of the pixels change with one more iteration")
        assert beyond > 0.0, "no leaf is found in the first iteration that the limit forbids"
    _check(family, limited, cam, ref, f"max_iter {max_iter}")


# ---- the bounce limit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_bounce", [1, 2, 8])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_bounce_limit(oracle, monkeypatch, family, max_bounce):
    """A lane that scatters at the limit ends in the same event pass."""
    _env(monkeypatch, family)
    scene, corner, block = _placed(family)
    cam = _outside(corner, block, bounce=max_bounce)
    ref = oracle.render(scene, cam, threads=8)
    more = dc.differ(ref, oracle.render(scene, _outside(corner, block, bounce=max_bounce + 1), threads=8))
    assert more > 0.0, "no path reaches the bounce limit"
    _check(family, scene, cam, ref, f"max_bounce {max_bounce}")


# ---- frame sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(2, 2), (33, 33), (96, 64)], ids=["2x2", "33x33", "96x64"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_frame_sizes(oracle, monkeypatch, family, size):
    """One partial wave, several waves, more pixels than one block has lanes."""
    _env(monkeypatch, family)
    scene, corner, block = _placed(family)
    cam = _inside(corner, block, w=size[0], h=size[1])
    _check(family, scene, cam, oracle.render(scene, cam, threads=8), "%dx%d" % size)


# ---- two-phase, progressive and replay frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_two_phase_frame(oracle, monkeypatch, family):
    """16 spp: a probe launch, then the rest in cost order; the phase events show the probe launch."""
    _env(monkeypatch, family)
    monkeypatch.setenv("TDT_TWO_PHASE_MIN_SPP", "16")
    row, geometry, _ = FAMILIES[family]
    scene, corner, block = _placed(family)
    cam = _outside(corner, block, spp=16)
    ref = oracle.render(scene, cam, threads=8)
    r = rt.Renderer(scene, cam)
    try:
        r.ctx.phase_timing(True)
        first = r.render()
        probe_ms, main_ms, _ = r.ctx.phase_timing(True)
        v = r.ctx.last_variant()
        again = r.render()
    finally:
        r.close()
    assert probe_ms > 0 and main_ms > 0, "the frame was not traced in two phases"
    assert (v["form"], v["depth"], v["resident"], v["full"], v["brick"], v["unit"]) == row + (1,) and (v["block"], v["per_cu"]) == geometry
    dr._assert_frame(first, ref, "first frame")
    dr._assert_frame(again, ref, "replay")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_progressive_frame(oracle, monkeypatch, family):
    """tdt_dispatch_accumulate twice, then tdt_dispatch_resolve: the records and the sums go through the caller's carry and image."""
    import torch
    _env(monkeypatch, family)
    row, geometry, _ = FAMILIES[family]
    scene, corner, block = _placed(family)
    cam = _outside(corner, block)
    ref = _oracle(oracle, scene, cam)
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    carry = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r = rt.Renderer(scene, cam, image_ptr=accum.data_ptr())
    try:
        r.shader.dispatch_accumulate(W + 1, H + 1, 1, 0, 1, carry.data_ptr())
        v = r.ctx.last_variant()
        r.shader.dispatch_accumulate(W + 1, H + 1, 1, 1, SPP - 1, carry.data_ptr())
        r.shader.dispatch_resolve(W + 1, H + 1, 1, SPP)
        img = r.texture.read()
    finally:
        r.close()
    assert (v["form"], v["depth"], v["resident"], v["full"], v["brick"], v["unit"]) == row + (1,) and (v["block"], v["per_cu"]) == geometry
    dr._assert_frame(img, ref, "progressive frame")


# ---- the statistics build --------------------------------------------------------------------------------------------------------
def _stats_child(depth, four, tmp_path):
    out = str(tmp_path / f"stats_{depth}_{int(four)}.npz")
    env = {**os.environ, "TDT_LIB": build.STATS_LIB, "TDT_PIXEL_LOG": "1"}
    env.pop("TDT_FOUR_WAVES", None)
    if four:
        env["TDT_FOUR_WAVES"] = "1"
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_bookkeeping_stats_frame.py"), str(depth), out],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]), np.load(out)


@pytest.mark.parametrize("depth", [5, 6])
def test_statistics_build_counts_the_same_passes(oracle, depth, tmp_path):
    """An 8 x 8 frame is one wave, so its pass statistics are deterministic.  Every ray leaves the traversal exactly once, through a
    leaf (the hit rows) or out of the octree / of iterations; every path ends exactly once (the end rows).  The oracle counts the
    same events: rays (OctreeHit calls), hits (material fetches), paths (samples).  The 256 x 5 build and the 1024 x 1 control run
    the same passes.  The cost a pixel records is 64 per event + 7 per traversal step of its rays (the step that ends a ray
    included), with the events and steps taken from the instrumented launch's per-pixel log."""
    assert os.path.exists(build.STATS_LIB), "build() makes the statistics library"
    scene = five._scene(depth, "reference_corner")
    cam = five._camera("reference_corner", 8, 8, SPP)
    ref, ost = oracle.render(scene, cam, threads=1, want_stats=True)
    hits = ost["lambertian"] + ost["metal"] + ost["dielectric"] + ost["unknown_material"]
    assert 0 < hits < ost["octree_hit_calls"], "the frame needs rays that hit and rays that leave"
    got = {}
    for four in (False, True):
        st, z = _stats_child(depth, four, tmp_path)
        got[four] = st
        assert (st["block"], st["per_cu"]) == (FOUR if four else FIVE) and st["full"] == 1 and st["waves"] >= 1
        dr._assert_frame(z["image"], ref, "statistics build")
        print(f"depth {depth} {'1024 x 1' if four else '256 x 5'}: {st}")
        assert st["newray_lanes"] == ost["octree_hit_calls"]
        assert st["hit_lanes"] == hits                                    # left through a leaf
        assert st["end_lanes"] == ost["samples"]                          # every path ends once
        cost, steps, events = z["cost"].astype(np.int64), z["steps"].astype(np.int64), z["events"].astype(np.int64)
        live = cost != 0
        assert live.sum() == 64 and ((steps != 0) == live).all()
        assert (cost[live] == 64 * events[live] + 7 * steps[live]).all(), (cost[live][:8], events[live][:8], steps[live][:8])
    for k in ("trav_pass", "trav_lanes", "inside_lanes", "event_pass", "hit_pass", "hit_lanes", "end_pass", "end_lanes"):
        assert got[False][k] == got[True][k], k
