"""The whole-depth builds at five waves per SIMD (csrc/tdt_rt.hip trace_kernel, kCold): 256-thread blocks, five to a CU, no node
table in LDS — the band fallback walks the cells in global memory — and the per-pixel state that only event passes touch (the two
hit records, the root call site's t, the running sums, the pixel's cost and coordinates) in per-lane LDS slots.

Every case is compared bit for bit with the oracle, on the depth-5 and depth-6 trees of test_gpu_full_grid_corners (EMPTY and
LEAF cells at every level, finest cells at digits 0 and 2^D - 1) in the three placements of test_gpu_plane_table (the UNIT build
and the multiplying build) and a fourth, the corner with a +0 and a -0 component at scale 2."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import degenerate_cams
import test_gpu_full_grid_corners as corners
import test_gpu_plane_table as planes
import tree_model
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu

POW2 = 1
BOUNCE = 4
# (width, height, spp).  2 x 2: fewer pixels than one block has lanes, so the queue is dry from the first draw
SIZES = {"96x64": (96, 64, 4), "33x33": (33, 33, 4), "2x2": (2, 2, 4)}
FIVE, FOUR = (256, 5), (1024, 1)
# name: (corner, scale, unit build)
PLACEMENTS = {**planes.PLACEMENTS, "zero_corner_scale_2": ((0.0, -0.0, -1.0), 2.0, 0)}

_refs = {}


def _scene(depth, placement, cells=None):
    corner, scale, _ = PLACEMENTS[placement]
    like = host.Scene.config(2)
    scene = tree_model.scene_from_cells(corners._tree(depth) if cells is None else cells, depth, 1 << 16, like, min_point=corner, scale=scale)
    return tree_model.with_corner(scene, np.array(corner, np.float32))            # (bit for bit: -0.0 stays -0.0)


def _camera(placement, w, h, spp):
    """test_gpu_plane_table's eye (the reference pose relative to the octree, looking along +x) for any image size."""
    corner, scale, _ = PLACEMENTS[placement]
    f32 = np.float32
    o = np.array(corner, f32) + np.array([0.5, 0.4, 0.7], f32) * f32(scale)
    d, right, up = np.array([1, 0, 0], f32), np.array([0, 0, 1], f32), np.array([0, 1, 0], f32)
    vh = f32(2.0)
    hor, ver = right * (f32(w) / f32(h) * vh), up * vh
    llc = o - hor * f32(0.5) - ver * f32(0.5) + d
    u = host.CameraUniforms()
    u.image_width, u.image_height, u.samples_per_pixel, u.max_bounce = w, h, spp, BOUNCE
    for name, v in (("horizontal", hor), ("vertical", ver), ("lower_left_corner", llc), ("origin", o)):
        getattr(u, name)[:] = [float(x) for x in v.astype(f32)]
    return u


def _ref(oracle, depth, placement, w, h, spp):
    key = (depth, placement, w, h, spp)
    if key not in _refs:
        ref = oracle.render(_scene(depth, placement), _camera(placement, w, h, spp), threads=4)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _geometry(v):
    return (v["block"], v["per_cu"])


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("depth", [5, 6])
def test_first_frame_and_replay_equal_the_oracle(oracle, depth, placement, size):
    w, h, spp = SIZES[size]
    ref = _ref(oracle, depth, placement, w, h, spp)
    r = rt.Renderer(_scene(depth, placement), _camera(placement, w, h, spp))
    try:
        first = r.render()
        v1 = r.ctx.last_variant()
        again = r.render()                            # the cost-ordered replay
        v2 = r.ctx.last_variant()
    finally:
        r.close()
    want = (POW2, depth, 1, 1, 0, PLACEMENTS[placement][2])
    for v in (v1, v2):
        assert planes._variant(v) == want and _geometry(v) == FIVE
    corners._same(first, ref, "first frame")
    corners._same(again, ref, "replay")


@pytest.mark.parametrize("placement", ["reference_corner", "scale_2", "zero_corner_scale_2"])
def test_two_phase_frame(oracle, monkeypatch, placement):
    """16 spp: a probe launch, then the rest in cost order.  The hit records travel LDS slots -> carry in memory -> LDS slots
    between the two launches.  That the frame had both launches is read from the phase events (a one-launch frame has no probe time)."""
    monkeypatch.setenv("TDT_TWO_PHASE_MIN_SPP", "16")
    depth, (w, h, spp) = 6, (96, 64, 16)
    ref = _ref(oracle, depth, placement, w, h, spp)
    r = rt.Renderer(_scene(depth, placement), _camera(placement, w, h, spp))
    try:
        r.ctx.phase_timing(True)
        first = r.render()
        probe_ms, main_ms, _ = r.ctx.phase_timing(True)
        v = r.ctx.last_variant()
        again = r.render()
    finally:
        r.close()
    assert probe_ms > 0 and main_ms > 0, "the frame was not traced in two phases"
    assert v["full"] == 1 and _geometry(v) == FIVE
    corners._same(first, ref, "first frame")
    corners._same(again, ref, "replay")


def test_progressive_frame(oracle):
    """tdt_dispatch_accumulate twice, then tdt_dispatch_resolve: sums and records through the image and the caller's carry."""
    import torch
    depth, placement, (w, h, spp) = 6, "reference_corner", (96, 64, 4)
    ref = _ref(oracle, depth, placement, w, h, spp)
    accum = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    carry = torch.zeros((h, w, 16), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r = rt.Renderer(_scene(depth, placement), _camera(placement, w, h, spp), image_ptr=accum.data_ptr())
    try:
        r.shader.dispatch_accumulate(w + 1, h + 1, 1, 0, 1, carry.data_ptr())
        v = r.ctx.last_variant()
        r.shader.dispatch_accumulate(w + 1, h + 1, 1, 1, spp - 1, carry.data_ptr())
        r.shader.dispatch_resolve(w + 1, h + 1, 1, spp)
        img = r.texture.read()
    finally:
        r.close()
    assert v["full"] == 1 and _geometry(v) == FIVE
    corners._same(img, ref, "progressive frame")


def _plane_bundle(depth):
    """Every primary ray lies in the plane x = corner + k 2^-depth with d_x = +0 (degenerate_cams.plane_bundle): every sample point of
    every primary ray has 2^depth (w_x - corner_x) = k, an integer, which is inside the band whatever its width."""
    k = (1 << depth) // 2 - 5
    x = degenerate_cams.face_coordinate(k, depth)
    assert float(np.float32(x - np.float32(-0.5))) * (1 << depth) == k
    cam = degenerate_cams.plane_bundle(0, (x, -0.1, -0.3), w=96, h=64, spp=4, bounce=BOUNCE)
    assert degenerate_cams.axis_component_bits(cam, 0) == [0]             # d_x = +0 for every pixel and sample
    return cam


@pytest.mark.parametrize("depth", [5, 6])
def test_rays_that_walk_global_memory(oracle, depth, tmp_path):
    """Rays whose sample points fall inside the x bands, so that their steps take the level-by-level walk — in this build, from
    global memory.  That the walk ran is read from the device: the statistics build of the library (libtdtrt_stats.so, loaded by a
    process of its own: a library is chosen when the package is imported) counts the traversal passes that take it.  Both builds
    render the oracle's bits."""
    cam = _plane_bundle(depth)
    scene = _scene(depth, "reference_corner")
    ref = oracle.render(scene, cam, threads=4)
    share = degenerate_cams.differ(ref, oracle.render(degenerate_cams.empty_tree(scene), cam, threads=4))
    assert share >= 0.1, f"the tree is not in view: {share:.3f}"
    r = rt.Renderer(scene, cam)
    try:
        first = r.render()
        v = r.ctx.last_variant()
        again = r.render()
    finally:
        r.close()
    assert planes._variant(v) == (POW2, depth, 1, 1, 0, 1) and _geometry(v) == FIVE
    corners._same(first, ref, "first frame")
    corners._same(again, ref, "replay")
    assert os.path.exists(build.STATS_LIB), "build() makes the statistics library"
    out = str(tmp_path / "stats_frame.npy")
    env = {**os.environ, "TDT_LIB": build.STATS_LIB}
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "five_waves_stats_frame.py"), str(depth), out],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    st = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert (st["block"], st["per_cu"]) == FIVE and st["full"] == 1
    print(f"depth {depth}: {st['fallback_pass']} of {st['trav_pass']} traversal passes took the walk, {st['fallback_lanes']} lanes in a band")
    assert st["fallback_pass"] > 0 and st["fallback_lanes"] > 0, st
    # every primary ray's steps are in a band, and a 96 x 64 frame at 4 spp has 24 576 of them: far more lanes than scattered rays could bring
    assert st["fallback_lanes"] >= 96 * 64 * 4, st
    corners._same(np.load(out), ref, "statistics build")


def test_frame_after_an_edit_of_a_leaf(oracle):
    """tdt_buffer_sub_data turns a finest-level LEAF in view into EMPTY: the walk reads the bound buffer itself, the table is rebuilt."""
    depth, placement, (w, h, spp) = 6, "reference_corner", SIZES["96x64"]
    scene, cam = _scene(depth, placement), _camera(placement, w, h, spp)
    before = _ref(oracle, depth, placement, w, h, spp)
    vox = corners._voxels(depth)
    half = 1 << (depth - 1)
    loose = vox[(vox[:, 0] >= half) & (vox[:, 1] >= half) & (vox[:, 2] < half)][:, :3]      # octant (1, 1, 0): in front of the camera
    for q in loose[:60]:
        node, level = corners._node_of(scene.blobs[0], depth, q)
        if level != depth or scene.blobs[0][2 * node + 1] != corners.LEAF:
            continue
        cells = scene.blobs[0].copy()
        cells[2 * node: 2 * node + 2] = 0
        after = oracle.render(_scene(depth, placement, cells), cam, threads=4)
        if (after.view(np.uint32) != before.view(np.uint32)).any():
            break
    else:
        raise AssertionError("no finest-level LEAF in view")
    r = rt.Renderer(scene, cam)
    try:
        corners._same(r.render(), before, "before the edit")
        r.vbos[0].sub_data(8 * node, np.zeros(2, np.uint32))
        img = r.render()
        v = r.ctx.last_variant()
    finally:
        r.close()
    assert v["full"] == 1 and _geometry(v) == FIVE
    corners._same(img, after, "after the edit")


@pytest.mark.parametrize("mode", [17, 18])
@pytest.mark.parametrize("depth", [5, 6])
def test_table_selftests(depth, mode):
    r = rt.Renderer(_scene(depth, "reference_corner"), _camera("reference_corner", 33, 33, 4))
    try:
        r.render()
        assert r.ctx.selftest(mode) == 0
    finally:
        r.close()


@pytest.mark.parametrize("placement", ["reference_corner", "zero_corner"])
def test_switch_selects_the_four_wave_build(oracle, monkeypatch, placement):
    """256 x 5 by default, 1024 x 1 under TDT_FOUR_WAVES=1 (read when the context is created); the same bits."""
    depth, (w, h, spp) = 6, SIZES["96x64"]
    ref = _ref(oracle, depth, placement, w, h, spp)
    imgs = {}
    for name, want in (("five", FIVE), ("four", FOUR)):
        if name == "four":
            monkeypatch.setenv("TDT_FOUR_WAVES", "1")
        r = rt.Renderer(_scene(depth, placement), _camera(placement, w, h, spp))
        try:
            imgs[name] = r.render()
            v = r.ctx.last_variant()
        finally:
            r.close()
        assert planes._variant(v) == (POW2, depth, 1, 1, 0, PLACEMENTS[placement][2])
        assert _geometry(v) == want, name
        corners._same(imgs[name], ref, name)
    assert (imgs["five"].view(np.uint32) == imgs["four"].view(np.uint32)).all()
