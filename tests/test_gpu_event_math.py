"""The arithmetic of a path event (scatter and primary ray) against the oracle's bits, where its short forms have their edges.

q_sqrt / q_rsq (csrc/trace_device.hpp) draw one hardware seed per square root and take the IEEE expression outside an exponent
window; ScatterDielectric feeds them, q_rcp and schlick_q with whatever the dielectric buffer holds.  The scenes here are small
trees of glass, metal and Lambert voxels whose dielectric entries sit on every branch of those guards (1.0, zeros of both signs, a
denormal, both sides of the window, inf, NaN, an `attribute` past the end of the buffer, an empty buffer), rendered by a
general-kernel build, the small-tree build, a whole-depth (FULL) build and a brick build, at image sizes whose primary-ray divisors
are 63, 32 and 1, and across the buffer's lifecycle (sub-data, re-bind).  The exhaustive comparison of the forms themselves with
the IEEE expressions is tdt_selftest modes 1 and 2 (tests/test_gpu_api.py)."""
import numpy as np
import pytest

from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

LITERAL, POW2 = 0, 1
LEAF = 2
F32 = np.float32
# 1.5, 1.0, 0, -0, a denormal, 2^-101 and 2^101 (outside the exponent window of the short forms), inf, NaN
IRS = np.array([0x3FC00000, 0x3F800000, 0x00000000, 0x80000000, 0x00000123, 0x0D000000, 0x72000000, 0x7F800000, 0x7FC00000], np.uint32).view(F32)
N_MATERIALS = 16


def glass_scene(cfg=1, irs=IRS):
    """Scene.config(cfg)'s tree with its leaves spread over 16 materials: 3 Lambert, 3 metal, one dielectric per entry of `irs`
    (as far as 9 go) and one dielectric whose attribute points one past the nine entries."""
    base = host.Scene.config(cfg)
    blobs = {k: v.copy() for k, v in base.blobs.items()}
    mats = [(0, 0, 0), (1, 0, 1), (1, 2, 2), (0, 0, 3), (1, 3, 0), (0, 0, 2)]
    mats += [(2, a, 0) for a in range(9)] + [(2, 9, 0)]
    assert len(mats) == N_MATERIALS
    blobs[1] = np.array(mats, np.uint32).reshape(-1)
    blobs[4] = np.ascontiguousarray(irs, F32)
    nodes = blobs[0].reshape(-1, 2)
    leaf = nodes[:, 1] == LEAF
    idx = np.nonzero(leaf)[0].astype(np.uint64)
    nodes[leaf, 0] = ((idx * np.uint64(2654435761)) >> np.uint64(7)).astype(np.uint32) % np.uint32(N_MATERIALS)
    return host.Scene(blobs, base.counts, f"glass{cfg}")


def differing(got, ref):
    return int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())


def render_gpu(scene, cam):
    r = rt.Renderer(scene, cam)
    try:
        img = r.render()
        return img, r.ctx.last_variant()
    finally:
        r.close()


CAMS = {64: (64, 64), 33: (33, 33), 2: (2, 2)}


@pytest.fixture(scope="module")
def scene1():
    return glass_scene(1)


@pytest.mark.parametrize("size", [64, 33, 2])
def test_glass_scene_small_tree(oracle, scene1, size):
    """depth-3 tree, 4 spp, max_bounce 8; the divisors of the primary ray are 63, 32 and 1"""
    cam = host.camera_reference_pose(size, size, 4, 8)
    assert (cam.image_width, cam.image_height) == CAMS[size]
    got, v = render_gpu(scene1, cam)
    ref = oracle.render(scene1, cam, threads=4)
    assert (v["form"], v["depth"]) == (POW2, 3)
    assert differing(got, ref) == 0
    if size == 64:                                      # the scene does what it is for: glass paths end in every kind of pixel
        assert np.isfinite(ref[..., :3]).all() and len(np.unique(ref.view(np.uint32)[..., 0])) > 200


def test_empty_dielectric_buffer(oracle):
    """every dielectric material reads past the end: ir = 0"""
    scene = glass_scene(1, irs=np.zeros(0, F32))
    cam = host.camera_reference_pose(64, 64, 4, 8)
    got, _ = render_gpu(scene, cam)
    assert differing(got, oracle.render(scene, cam, threads=4)) == 0


def test_glass_scene_general_kernel(oracle, monkeypatch):
    """a cell_count that is not a power of two, its threshold builds switched off: the literal-formula kernel"""
    monkeypatch.setenv("TDT_NO_TABLE_FORM", "1")
    scene = host.scene_with_cell_count(glass_scene(1), 100000)
    cam = host.camera_reference_pose(64, 64, 4, 8)
    got, v = render_gpu(scene, cam)
    assert (v["form"], v["depth"]) == (LITERAL, 0)
    assert differing(got, oracle.render(scene, cam, threads=4)) == 0


@pytest.mark.parametrize("cfg,full,brick", [(2, 1, 0), (3, 0, 1)])
def test_glass_scene_full_and_brick_builds(oracle, cfg, full, brick):
    scene = glass_scene(cfg)
    cam = host.camera_reference_pose(64, 64, 4, 8)
    got, v = render_gpu(scene, cam)
    assert (v["form"], v["full"], v["brick"]) == (POW2, full, brick)
    assert differing(got, oracle.render(scene, cam, threads=4)) == 0


def test_dielectric_buffer_lifecycle(oracle, scene1):
    """render; change one ir in place; render; bind another buffer to the slot; render — each frame is the oracle's for the values
    then bound (whatever a build derives from the buffer follows its contents)"""
    cam = host.camera_reference_pose(64, 64, 4, 8)
    r = rt.Renderer(scene1, cam)
    try:
        first = r.render()
        assert differing(first, oracle.render(scene1, cam, threads=4)) == 0
        irs2 = IRS.copy(); irs2[0] = F32(2.4)
        r.vbos[4].sub_data(0, irs2[:1])
        s2 = glass_scene(1, irs=irs2)
        ref2 = oracle.render(s2, cam, threads=4)
        assert differing(ref2, oracle.render(scene1, cam, threads=4)) > 0      # the change shows
        assert differing(r.render(), ref2) == 0
        irs3 = np.array([1.1, 1.3, 1.7], F32)           # shorter: attributes 3..9 now point past the end
        other = rt.VertexBufferObject(r.ctx, irs3)
        r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 4, other)
        ref3 = oracle.render(glass_scene(1, irs=irs3), cam, threads=4)
        assert differing(ref3, ref2) > 0                # the re-bind shows
        assert differing(r.render(), ref3) == 0
    finally:
        r.close()

