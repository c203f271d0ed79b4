"""The oracle against the reference shader's own frames (llvmpipe) of axis-parallel ray bundles lying in cell-face planes:
tests/golden/degenerate/*.npz, made by oracle/make_goldens.py --degenerate from the cases of tests/degenerate_cams.py.  On these
rays the slab operands are +-inf and 0 * inf = NaN, so the fixtures pin the oracle's min/max NaN rule ("a NaN operand yields the
other one"), which tests/test_oracle_golden.py's NaN-free frames leave open.  Bit-exact."""
import hashlib
import json
import os

import numpy as np
import pytest

import degenerate_cams as dc
import tree_model
from tdt4230_project_raytracing_amd import host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "degenerate")
NAMES = sorted(dc.FIXTURES)


def load(name):
    """(reference image, meta, scene, camera as the reference was sent it) of a fixture."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    scene = dc.fixture_scene(tuple(meta["scene"]), z["corner_bits"].view(np.float32))
    cam = dc.camera_from_bits(z["camera_bits"], meta["W"], meta["H"], meta["spp"], meta["max_bounce"])
    return z["image"], meta, scene, cam


def test_every_case_has_its_fixture():
    assert sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) == NAMES and len(NAMES) >= 16


@pytest.mark.parametrize("name", NAMES)
def test_scene_and_camera_reproduce(name):
    """The case's parameters give, today, the bytes the reference rendered: every scene payload and all twelve camera floats
    (-0 and denormals included)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    _, meta, stored_scene, stored_cam = load(name)
    scene, cam, axis, kind = dc.fixture_case(name)
    assert (axis, kind, list(dc.FIXTURES[name][0])) == (meta["axis"], meta["kind"], meta["scene"])
    for s in (scene, stored_scene):
        for slot, digest in meta["scene_sha256"].items():
            assert hashlib.sha256(np.ascontiguousarray(s.blobs[int(slot)]).tobytes()).hexdigest() == digest, f"payload {slot}"
    assert dc.camera_bits(cam).tolist() == z["camera_bits"].tolist() == dc.camera_bits(stored_cam).tolist()
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_bounce) == (meta["W"], meta["H"], meta["spp"], meta["max_bounce"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_bit_exact_and_premises(oracle, name):
    golden, meta, scene, cam = load(name)
    axis, kind = meta["axis"], meta["kind"]
    img, st, share = dc.premises(oracle, scene, cam, axis, kind)
    print(f"{name}: nan_slab_tests {st['nan_slab_tests']} inf_slab_tests {st['inf_slab_tests']} view share {share:.3f}")
    eq = (img.view(np.uint32) == golden.view(np.uint32)).all(axis=2)
    assert eq.all(), f"{int((~eq).sum())} of {eq.size} pixels differ from the reference render"
    # what the case claims about the direction itself
    bits = dc.axis_component_bits(cam, axis)
    if "negzero" in name:
        assert bits == [0x80000000]
    elif "tiny" in name:
        assert 0x00800000 <= max(bits) < 0x0D800000        # normal, and below the reciprocal's fast window (2^-100)
    elif "denormal" in name:
        assert 0 < max(bits) < 0x00800000
    else:
        assert bits == [0]
    if "minface" in name:                     # the bundle lies in the octree's own min face: 0 * inf at the root test as well
        assert scene.blobs[6][axis] == 0 and cam.origin[axis] == 0
        assert bool(np.signbit(np.float32(cam.origin[axis]))) == name.endswith("neg")


def test_counters_sit_at_the_end_of_the_stats():
    import oracle_py
    assert oracle_py.STAT_FIELDS[:9] == ["pixels", "samples", "octree_hit_calls", "iterations", "node_loads", "lambertian", "metal",
                                         "dielectric", "unknown_material"]
    assert oracle_py.STAT_FIELDS[9:] == ["nan_slab_tests", "inf_slab_tests"]


def test_face_coordinate_is_the_traversals_cell_corner(oracle):
    """fl(fl(k / 2^depth * scale) + min), also for a scale that is not 1 and a placed corner: the arithmetic, and its effect — an
    origin there equals the corner of the cells above the plane bit for bit, which is what gives 0 * inf."""
    f32 = np.float32
    for k, depth, scale, mn in ((27, 6, 1.0, -0.5), (27, 6, 2.5, 0.3), (123, 8, 0.7, -1.5), (1019, 10, 1.0, 0.75), (5, 3, 3.3, 0.1)):
        g = f32(0.0)
        for level in range(1, depth + 1):     # treeLookup's sum of bits * 2^-level (raytracer.comp:380)
            g = f32(g + f32((k >> (depth - level)) & 1) * f32(2.0 ** -level))
        assert dc.face_coordinate(k, depth, scale, mn) == f32(f32(g * f32(scale)) + f32(mn))
    like = host.Scene.config(2)
    mn, scale = np.array([0.3, -1.7, 0.2], f32), f32(0.7)
    scene = tree_model.scene_from_cells(like.blobs[0], like.max_depth, like.cell_count, like, min_point=mn, scale=scale)
    y = dc.face_coordinate(dc.K6, 6, scale, mn[1])
    cam = dc.plane_bundle(1, (mn[0] + scale * f32(0.5), y, mn[2] + scale * f32(0.7)))
    assert oracle.render(scene, cam, threads=8, want_stats=True)[1]["nan_slab_tests"] >= dc.NAN_TESTS


def test_the_fixtures_that_go_through_the_miss_pre_pass(oracle):
    """The library runs the miss pre-pass before every frame of a camera outside the octree, whatever the sample count
    (tdt_dispatch_compute).  Two fixtures stand there, one of them a two-phase frame, and in both the pre-pass has pixels to finish:
    some of the frame is the sky an empty tree gives."""
    out = [n for n in NAMES if dc.outside(*load(n)[2:])]
    assert out == ["config2_yplane_outside", "config2_yplane_outside_spp16"]
    assert [load(n)[1]["spp"] for n in out] == [3, 16]
    for n in out:
        golden, _, scene, cam = load(n)
        sky = 1.0 - dc.differ(golden, oracle.render(dc.empty_tree(scene), cam, threads=8))
        assert sky >= 0.02, sky


@pytest.mark.parametrize("view", [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)], ids=["along+x", "along-x"])
def test_z_plane_bundle(oracle, view):
    """plane_bundle on z (the view along +-x; no fixture has one: config 2's z planes leave too little in view).  Every ray has
    d_z == +0, on the face and off it, and the frame meets +-inf slab operands; on the face plane it meets 0 * inf as well."""
    scene = host.Scene.config(2)
    z = dc.face_coordinate(dc.K6, 6, 1.0, -1.0)
    for cam, on_face in ((dc.plane_bundle(2, (0.3 * -view[0], -0.1, z), view=view), True),
                         (dc.plane_bundle(2, (0.3 * -view[0], -0.1, -0.55), view=view), False)):
        assert dc.axis_component_bits(cam, 2) == [0]
        assert cam.horizontal[:] == [0.0, 0.0, 0.0] and cam.vertical[2] == 0 and cam.lower_left_corner[2] == cam.origin[2]
        st = oracle.render(scene, cam, threads=8, want_stats=True)[1]
        assert st["inf_slab_tests"] > 0
        assert (st["nan_slab_tests"] > 0) == on_face, st["nan_slab_tests"]
