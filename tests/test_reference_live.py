"""The oracle against the reference shader on scenes and cameras the other fixtures do not hold: fresh generated scenes, other
cell counts, turned cameras, fresh presentation frames, and the shader's work-group size and buffer layout.  The reference's
answers were recorded on llvmpipe (oracle/make_goldens.py --live) into tests/golden/live/reference_live.npz; the inputs are rebuilt
here from their parameters."""
import json
import os

import numpy as np
import pytest

import make_goldens as mg
from tdt4230_project_raytracing_amd import host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live", "reference_live.npz")


@pytest.fixture(scope="module")
def live():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


@pytest.mark.parametrize("kind,depth,seed", mg.LIVE_FRESH)
def test_oracle_vs_reference_shader_fresh_scene(oracle, live, kind, depth, seed):
    scene = host.Scene.generate(kind, depth, 1 << 14, 100, seed)
    cam = host.camera_reference_pose(96, 64, 2, 5)
    ref = live[0][f"fresh_{kind}_{depth}_{seed}"]
    got = oracle.render(scene, cam, threads=4)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("kind,depth,seed,cc", mg.LIVE_CELL_COUNTS)
def test_oracle_vs_reference_shader_under_other_cell_counts(oracle, live, kind, depth, seed, cc):
    """cell_count as the reference's own host passes it (100000: not a power of two) and neighbours of it: the index arithmetic of
    treeLookup then reads the previous cell at the bottom of many cells — against the shader on fresh scenes, rays along cell
    boundaries included."""
    scene = host.scene_with_cell_count(host.Scene.generate(kind, depth, 1 << 20, 100, seed), cc, 1000)
    for i, origin in enumerate(mg.LIVE_CC_ORIGINS):
        cam = mg.live_cc_camera(origin)
        ref = live[0][f"cc_{kind}_{depth}_{seed}_{cc}_{i}"]
        got = oracle.render(scene, cam, threads=4)
        assert (got.view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("cfg,origin,yaw,pitch,fov", mg.LIVE_TURNED)
def test_oracle_vs_reference_shader_turned_camera(oracle, live, cfg, origin, yaw, pitch, fov):
    """Turned cameras (camera.rs:68-82: every component of horizontal / vertical / lower_left_corner non-zero but horizontal.y, which the
    controller keeps at 0), inside the octree and outside looking in: the uniforms of the host's controller mirror, whatever their
    last bit, through the shader and the oracle.  (The controller turns by 2 * angle * turn_rate radians, turn_rate 0.025.)"""
    scene = host.Scene.config(cfg)
    cam = mg.live_turned_camera(origin, yaw, pitch, fov)
    assert sum(abs(x) > 1e-3 for v in (cam.horizontal, cam.vertical, cam.lower_left_corner) for x in v) >= 8
    ref = live[0][f"turned_{cfg}"]
    got = oracle.render(scene, cam, threads=4)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()


def test_reference_work_group_size_and_layout(live):
    """compute_shader.rs:18 queries {32,32,1}; the `layout(shared)` blocks are packed like std430,
    which is what the tightly packed host payloads assume (SURVEY.md §7 hard parts)."""
    meta = live[1]
    assert meta["group_size"] == [32, 32, 1]
    expect = {"indirect_cells[0].value": (0, 8), "indirect_cells[0].type": (4, 8),
              "octree_floats[0].scale": (16, None), "octree_floats[0].inv_scale": (20, None),
              "octree_floats[0].inv_cell_count": (24, None), "octree_ints[0].max_iter": (4, None),
              "octree_ints[0].cell_count": (8, None), "materials[0].albedo_index": (8, 12), "albedos[0].z": (8, 12)}
    for name, (off, stride) in expect.items():
        out = meta["buffer_variables"][name]
        assert out[0] == off, (name, out[0])
        if stride is not None:
            assert out[1] == stride, (name, out[1])


def test_presentation_vs_reference_quad_pass_fresh_frames(live):
    """quad.vert / quad.frag on llvmpipe against tdt_present_rgba8, on frames the other fixtures do not hold."""
    for (h, w), img in mg.live_present_frames().items():
        got = host.present_rgba8(img, top_down=False)
        assert (got == live[0][f"present_{h}x{w}"]).all(), (h, w)
