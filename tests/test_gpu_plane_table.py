"""The whole-depth table's plane form (csrc/trace_device.hpp PlaneTable, full_entry_planes; csrc/tdt_rt.hip build_full_grid_kernel):
a traversal step reads the cell's padded slab planes from a table every block builds in LDS, at byte offsets the table entry carries.

The device check of every table position (tdt_selftest 18: planes through the offsets against the arithmetic form, bit for bit) and
renders against the oracle, bit for bit, of the depth-5 and depth-6 trees of test_gpu_full_grid_corners (LEAF and EMPTY cells at
every level, finest-level cells in both far corners) in three placements of the octree: the reference's corner at scale 1 (the UNIT
build), a corner with a +0 and a -0 component at scale 1 and scale 2 (both the multiplying build).  The camera sits at the same
place relative to the octree in all of them and looks along +x."""
import numpy as np
import pytest

import test_gpu_full_grid_corners as corners
import tree_model
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

POW2 = 1
W, H, SPP, BOUNCE = 96, 64, 4, 4
# name: (corner, scale, unit build)
PLACEMENTS = {
    "reference_corner": ((-0.5, -0.5, -1.0), 1.0, 1),
    "zero_corner": ((0.0, -0.0, -1.0), 1.0, 0),
    "scale_2": ((-0.5, -0.5, -1.0), 2.0, 0),
}

_refs = {}


def _scene(depth, placement, cells=None):
    corner, scale, _ = PLACEMENTS[placement]
    like = host.Scene.config(2)
    scene = tree_model.scene_from_cells(corners._tree(depth) if cells is None else cells, depth, 1 << 16, like, min_point=corner, scale=scale)
    return tree_model.with_corner(scene, np.array(corner, np.float32))            # (bit for bit: -0.0 stays -0.0)


def _camera(placement):
    """The eye of the reference pose relative to the octree (main.rs:165-168: corner + (0.5, 0.4, 0.7) x scale), looking along +x."""
    corner, scale, _ = PLACEMENTS[placement]
    f32 = np.float32
    o = np.array(corner, f32) + np.array([0.5, 0.4, 0.7], f32) * f32(scale)
    d, right, up = np.array([1, 0, 0], f32), np.array([0, 0, 1], f32), np.array([0, 1, 0], f32)
    vh = f32(2.0)
    hor, ver = right * (f32(W) / f32(H) * vh), up * vh
    llc = o - hor * f32(0.5) - ver * f32(0.5) + d
    u = host.CameraUniforms()
    u.image_width, u.image_height, u.samples_per_pixel, u.max_bounce = W, H, SPP, BOUNCE
    for name, v in (("horizontal", hor), ("vertical", ver), ("lower_left_corner", llc), ("origin", o)):
        getattr(u, name)[:] = [float(x) for x in v.astype(f32)]
    return u


def _ref(oracle, depth, placement):
    key = (depth, placement)
    if key not in _refs:
        ref = oracle.render(_scene(depth, placement), _camera(placement), threads=4)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _variant(v):
    return (v["form"], v["depth"], v["resident"], v["full"], v["brick"], v["unit"])


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("depth", [5, 6])
def test_planes_through_the_offsets_equal_the_arithmetic(depth, placement):
    r = rt.Renderer(_scene(depth, placement), _camera(placement))
    try:
        assert r.ctx.selftest(18) == 0
    finally:
        r.close()


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("depth", [5, 6])
def test_render_equals_the_oracle(oracle, depth, placement):
    scene, cam = _scene(depth, placement), _camera(placement)
    ref = _ref(oracle, depth, placement)
    empty = host.Scene({**scene.blobs, 0: np.zeros(16, np.uint32)}, None, "empty")
    assert (ref.view(np.uint32) != oracle.render(empty, cam, threads=4).view(np.uint32)).any(axis=2).mean() >= 0.1, "the tree is not in view"
    r = rt.Renderer(scene, cam)
    try:
        first = r.render()
        v1 = r.ctx.last_variant()
        again = r.render()
        v2 = r.ctx.last_variant()
    finally:
        r.close()
    want = (POW2, depth, 1, 1, 0, PLACEMENTS[placement][2])
    assert v1["full"] == 1 and v2["full"] == 1
    assert _variant(v1) == want and _variant(v2) == want
    corners._same(first, ref, "first frame")
    corners._same(again, ref, "replay")


def test_render_after_an_edit_of_a_leaf(oracle):
    """tdt_buffer_sub_data turns one finest-level LEAF that the camera sees into EMPTY between two frames: the table is rebuilt (its
    key holds the buffer's version) and its new entry names the EMPTY cell's planes."""
    depth, placement = 6, "reference_corner"
    scene, cam = _scene(depth, placement), _camera(placement)
    before = _ref(oracle, depth, placement)
    vox = corners._voxels(depth)
    h = 1 << (depth - 1)
    loose = vox[(vox[:, 0] >= h) & (vox[:, 1] >= h) & (vox[:, 2] < h)][:, :3]          # octant (1, 1, 0): in front of the camera
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
        assert r.ctx.selftest(18) == 0
    finally:
        r.close()
    assert v["full"] == 1 and _variant(v) == (POW2, depth, 1, 1, 0, 1)
    corners._same(img, after, "after the edit")
