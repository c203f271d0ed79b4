"""The denoiser's numpy model (tests/denoise_model.py) on the CPU: its own rules on hand-made guides, and what it is for — on the
oracle's 4-spp frames of Scene.config(1) seen from inside it takes the error against 512 spp down by an order of magnitude."""
import numpy as np
import pytest

import denoise_model as model
from tdt4230_project_raytracing_amd import host


def _guide(kind, material=0, plane=0.0):
    kind = np.asarray(kind, np.uint32)
    g = np.zeros(kind.shape, model.GUIDE_DTYPE)
    g["kind"], g["material"], g["plane"] = kind, material, plane
    return g


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_pass_through_texels_are_copied_bitwise():
    rng = np.random.default_rng(1)
    img = rng.standard_normal((9, 11, 4)).astype(np.float32)
    img[2, 3] = [np.nan, np.inf, -0.0, 1e-41]
    img.view(np.uint32)[4, 4, 0] = 0x7FC12345                        # a NaN with a payload
    kind = rng.integers(0, 2, (9, 11))
    kind[2, 3] = kind[4, 4] = 0
    out = model.denoise(img, _guide(kind * 14), 3)
    hole = kind == 0
    assert (_bits(out)[hole] == _bits(img)[hole]).all()              # alpha included
    assert (_bits(out[..., 3]) == _bits(img[..., 3])).all()          # alpha is never filtered
    assert (_bits(out[..., :3])[~hole] != _bits(img[..., :3])[~hole]).any()


def test_regions_with_different_keys_never_mix():
    for other in ((14, 2, np.nextafter(np.float32(0.5), np.float32(1))), (14, 3, np.float32(0.5)), (15, 2, np.float32(0.5))):
        g = _guide(np.full((12, 16), 14), 2, np.float32(0.5))
        right = np.zeros((12, 16), bool)
        right[:, 8:] = True
        right[5, 2] = True                                            # and one texel of it inside the left region
        g["kind"][right], g["material"][right], g["plane"][right] = other
        img = np.where(right[..., None], np.float32(np.nan), np.float32(0.5)) * np.ones((12, 16, 4), np.float32)
        out = model.denoise(img, g, 4)
        assert np.isfinite(out[~right]).all() and (out[~right][:, :3] == 0.5).all()
        assert np.isnan(out[right][:, :3]).all()


def test_a_step_larger_than_the_image_leaves_the_centre_tap():
    rng = np.random.default_rng(2)
    img = rng.standard_normal((4, 4, 4)).astype(np.float32)
    g = _guide(np.full((4, 4), 14))
    assert (model.kept_taps(g, 4) == 1).all() and (model.kept_taps(g, 1) > 1).all()
    three = model.denoise(img, g, 2)
    # passes 2.. (steps 4, 8, ..) keep only the centre: out = (9/64 * v) / (9/64)
    w = np.float32(0.140625)
    want = three.copy()
    for _ in range(2):
        want[..., :3] = (w * want[..., :3]) / w
    assert (_bits(model.denoise(img, g, 4)) == _bits(want)).all()


def test_guide_from_hits_words():
    hit_dtype = np.dtype([("status", "<i4"), ("material", "<u4"), ("t", "<f4"), ("iterations", "<i4"), ("point", "<f4", (3,)),
                          ("normal", "<f4", (3,)), ("front_face", "<i4"), ("fresh_record", "<i4"), ("cell_min", "<f4", (3,)),
                          ("cell_size", "<f4")])
    h = np.zeros(7, hit_dtype)
    h["status"], h["fresh_record"], h["material"], h["t"] = 1, 1, [0, 1, 0, 0, 0, 5, 0], 2.5
    h["cell_min"], h["cell_size"] = [0.25, -0.5, 0.125], 0.0625
    h["normal"] = [[1, 0, 0], [0, -1, 0], [0, 0, 0], [0, 0.6, 0.8], [0, 0, -1], [0, 0, 1], [-1, 0, 0]]
    h["status"][4], h["fresh_record"][6] = 2, 0
    materials = np.array([[0, 0, 0], [1, 0, 1]], np.int32)            # entry 0 Lambertian, entry 1 metal, entry 5 past the end
    g = model.guide_from_hits(h, materials, False)
    assert list(g["kind"]) == [1 + 9 * 2 + 3 + 1, 0, 0, 1 + 9 + 3 * 2 + 2, 0, 0, 0]
    assert list(g["plane"]) == [np.float32(0.25) + np.float32(0.0625), 0, 0, np.float32(-0.5) + np.float32(0.0625), 0, 0, 0]
    assert list(g["material"]) == [0, 1, 0, 0, 0, 5, 0] and (g["t"] == 2.5).all()
    ga = model.guide_from_hits(h, None, True)
    assert list(ga["kind"]) == [23, 1 + 9 + 0 + 1, 0, 18, 0, 1 + 9 + 3 + 2, 0]
    assert ga["plane"][1] == np.float32(-0.5) and ga["plane"][5] == np.float32(0.125) + np.float32(0.0625)


# ---- what it is for --------------------------------------------------------------------------------------------------------
W, H, COVER = 240, 160, (256, 160)                   # (a dispatch whose 32x32 work-groups cover all of 240x160)
INSIDE_POSES = [((0.1, 0.05, -0.6), 135.0, 10.0, 70.0), ((0.0, -0.1, -0.3), 0.0, 0.0, 90.0)]
# raw / denoised mean squared error at 1, 2, 3 passes that this model measures at the two poses (240x160, 4 spp against 512 spp,
# max_bounce 8, linear means, over the kind != 0 pixels); DESIGN.md records them
MEASURED = ([7.93, 13.16, 14.07], [8.01, 12.11, 12.83])
MEASURED_AT_3 = (MEASURED[0][2], MEASURED[1][2])


def _cam(origin, yaw, pitch, fov, spp, bounce):
    c = host.Camera(fov, W, aspect_ratio=np.float32(W) / np.float32(H), origin=origin, viewport_height=2.0, samples_per_pixel=spp,
                    max_bounce=bounce)
    if yaw:
        c.turn_yaw(yaw)
    if pitch:
        c.turn_pitch(pitch)
    return c.uniforms()


def oracle_guide(oracle, scene, pose):
    """The guide of sample 0 from a one-sample, one-bounce oracle pass over the scene with every material made Lambertian with an
    albedo of its own (as tests/test_gpu_raycast.py reads a first hit): the colour names the material or the sky, the carry holds
    the record's normal and point.  The carry does not give cell_min, so the plane is keyed by the hit point rounded to the finest
    grid; and the record is the leaf call site's when that one is non-zero, else the root's."""
    n_mat = len(scene.blobs[1]) // 3
    mats = np.zeros((n_mat, 3), np.uint32)
    mats[:, 2] = np.arange(n_mat)
    i = np.arange(n_mat, dtype=np.float32)
    alb = np.stack([(i + 1) / np.float32(n_mat + 2), np.float32(1) - (i + 1) / np.float32(n_mat + 3), np.full(n_mat, 0.25, np.float32)], 1)
    blobs = dict(scene.blobs)
    blobs[1], blobs[2] = mats.reshape(-1), alb.astype(np.float32).reshape(-1)
    accum, carry = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 16), np.float32)
    oracle.accumulate(host.Scene(blobs, name=scene.name + "_lamb"), _cam(*pose, 1, 1), accum, carry, 0, 1, dispatch=COVER, threads=16)
    hit = _bits(accum[..., 2]) == _bits(np.float32(0.25))
    material = np.argmin(np.abs(accum[..., 0:1] - alb[None, None, :, 0]), -1)
    leaf = (carry[..., 8:11] != 0).any(-1)
    normal = np.where(leaf[..., None], carry[..., 8:11], carry[..., 0:3])
    point = np.where(leaf[..., None], carry[..., 12:15], carry[..., 4:7])
    types = np.ascontiguousarray(scene.blobs[1]).reshape(-1, 3).view(np.uint32)[:, 0]
    nonzero = normal != 0
    keyed = hit & nonzero.any(-1) & (types[material] == 0)
    s = np.where(normal < 0, 0, np.where(normal > 0, 2, 1))
    a = np.argmax(nonzero, -1)[..., None]
    floats, ints = np.asarray(scene.blobs[6], np.float32), np.asarray(scene.blobs[7], np.int32)
    cell = (np.take_along_axis(point, a, -1)[..., 0] - floats[:3][a[..., 0]]) / floats[4] * float(1 << int(ints[0]))
    g = np.zeros((H, W), model.GUIDE_DTYPE)
    g["kind"] = np.where(keyed, 1 + 9 * s[..., 0] + 3 * s[..., 1] + s[..., 2], 0)
    g["material"] = np.where(hit, material, 0)
    g["plane"] = np.where(keyed, np.rint(cell), 0).astype(np.float32)
    return g


def error_ratios(oracle, scene, pose, passes=(1, 2, 3)):
    """(raw / denoised mean squared error for each pass count, fraction of pass-through pixels)."""
    guide = oracle_guide(oracle, scene, pose)
    means = []
    for spp in (4, 512):
        acc = np.zeros((H, W, 4), np.float32)
        oracle.accumulate(scene, _cam(*pose, spp, 8), acc, None, 0, spp, dispatch=COVER, threads=16)
        means.append(acc / np.float32(spp))
    noisy, truth = means
    f = guide["kind"] != 0

    def mse(a):
        return float(np.mean((a[f][:, :3].astype(np.float64) - truth[f][:, :3]) ** 2))

    return [mse(noisy) / mse(model.denoise(noisy, guide, p)) for p in passes], 1.0 - float(f.mean())


@pytest.mark.parametrize("k", range(2))
def test_config1_from_inside_gets_much_cleaner(oracle, k):
    """4 spp against 512 spp on the CPU oracle, error over the kind != 0 pixels.  The guide keys the plane by the hit point rounded
    to the finest grid, not by cell_min (the oracle's carry does not hold it; see oracle_guide).  Measured: MEASURED above."""
    ratios, passed = error_ratios(oracle, host.Scene.config(1), INSIDE_POSES[k])
    print(f"pose {k}: raw/denoised MSE at 1, 2, 3 passes = {ratios}, pass-through {passed:.3f}")
    assert all(r > 1 for r in ratios)
    assert max(ratios) in ratios[1:]                                  # largest at 2 or 3 passes
    assert ratios[2] >= 0.5 * MEASURED_AT_3[k]                        # (the model is deterministic: the margin is room for a deliberate change of the key)
