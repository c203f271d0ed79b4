"""The numpy model of tdt_image_upsample (tests/upsample_model.py) without a GPU: the integer mapping stays inside the source, the
equal-size call is the identity, a linear ramp on one surface is reproduced by stage 1 alone, and every hand-made case the GPU test
runs reaches the classes it can — asserted here so that the GPU test cannot pass by never entering a stage."""
import time

import numpy as np
import pytest

import upsample_model as model
from denoise_model import GUIDE_DTYPE

F = np.float32


def _one_key(w, h):
    g = np.zeros((h, w), GUIDE_DTYPE)
    g["kind"], g["material"], g["plane"] = 14, 2, F(0.25)
    return g


def test_the_mapping_stays_inside_the_source():
    for W in range(1, 41):
        for w in range(1, W + 1):
            i0, i1, near, f = model.axis_map(W, w)
            assert i0.min() >= 0 and i1.max() <= w - 1, (W, w)
            assert ((i0 <= near) & (near <= i1)).all(), (W, w)
            assert ((i1 == i0 + 1) | (i1 == w - 1)).all(), (W, w)
            assert f.dtype == F and (f >= 0).all() and (f < 1).all(), (W, w)
            assert i0[0] == 0 and f[0] == 0 and i0[-1] == w - 1 and f[-1] == 0, (W, w)   # the corners of the two grids coincide
            if W == w:
                assert (i0 == np.arange(W)).all() and not f.any(), W


def test_the_mapping_is_the_floor_at_long_rows():
    for W, w in ((4097, 1366), (32768, 32767), (32768, 32768), (32768, 2)):
        i0, _, _, f = model.axis_map(W, w)
        x = np.arange(W, dtype=object)                                     # (Python integers: no width to overflow)
        assert (i0.astype(object) * (W - 1) <= x * (w - 1)).all() and ((i0.astype(object) + 1) * (W - 1) > x * (w - 1)).all()
        assert (f < 1).all()


def test_equal_sizes_and_equal_guides_are_the_identity():
    dst_guide, src, _ = model.make_case(64, 48, 64, 48, seed=21)
    src = np.where(np.signbit(src) & (src == 0), F(0.0), src)             # (no -0)
    out, cls = model.upsample(dst_guide, src, dst_guide)
    assert (cls == 1).all()
    assert out.view(np.uint32).tobytes() == src.view(np.uint32).tobytes()
    # stage 1 starts from +0: -0 comes back as +0 and nothing else changes
    src[3, 5] = F(-0.0)
    out, _ = model.upsample(dst_guide, src, dst_guide)
    assert not np.signbit(out[3, 5]).any() and not out[3, 5].any()
    rest = np.ones(src.shape, bool)
    rest[3, 5] = False
    assert out.view(np.uint32)[rest].tobytes() == src.view(np.uint32)[rest].tobytes()


def test_a_linear_ramp_on_one_surface_is_reproduced():
    w, h, W, H = 17, 9, 33, 17                                             # (W - 1) = 2 (w - 1): every fraction is 0 or 1/2, exact
    xs, ys = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    src = np.stack([xs, ys, F(3) * xs - F(2) * ys, xs + ys + F(1)], -1).astype(F)
    out, cls = model.upsample(_one_key(W, H), src, _one_key(w, h))
    assert (cls == 1).all()
    X, Y = np.meshgrid(np.arange(W, dtype=F) / F(2), np.arange(H, dtype=F) / F(2))
    want = np.stack([X, Y, F(3) * X - F(2) * Y, X + Y + F(1)], -1).astype(F)
    assert out.tobytes() == want.tobytes()


@pytest.mark.parametrize("case", model.HAND_CASES + [model.MULTI_CASE], ids=lambda c: "%dx%d<-%dx%d" % c[:4])
def test_the_hand_made_cases_reach_every_class(case):
    """A source of one texel cannot reach the ring: that texel is tap (i0, j0) of every pixel, whose weight (1 - fx)(1 - fy) is
    positive, so a pixel either keeps it (class 1) or finds it again, mismatching, in the ring (class 3).  2x2 <- 1x1 must reach
    both; 1x1 <- 1x1 is one pixel.  Every other case reaches all three."""
    W, H, w, h, seed = case
    dst_guide, src, src_guide = model.make_case(W, H, w, h, seed)
    t0 = time.perf_counter()
    out, cls, skipped = model.upsample(dst_guide, src, src_guide, with_skipped=True)
    took = time.perf_counter() - t0
    counts = model.histogram(cls)
    assert counts[0] == W * H == counts[1] + counts[2] + counts[3]
    if (w, h) == (1, 1):
        want = {1, 3} if W * H > 1 else {int(cls[0, 0])}
    else:
        want = {1, 2, 3}
    assert set(np.unique(cls).tolist()) == want, counts
    assert skipped[cls != 1].all()                                         # (a pixel that left stage 1 empty skipped all its taps)
    if (W, H) == (64, 48):
        assert took < 1.0, took
    if W * H > 100:                                                        # the special values are in the source, and some survive
        bits = src.view(np.uint32)
        assert np.isnan(src).any() and np.isinf(src).any() and (bits == 0x80000000).any() and ((bits & 0x7F800000) == 0)[src != 0].any()
        assert np.isnan(out).any() and np.isinf(out).any()


def test_kind_zero_is_a_key_like_any_other():
    """Sky interpolates among sky, a pass-through hit among pass-through hits of its material, and neither takes from the other."""
    src_guide = np.zeros((2, 2), GUIDE_DTYPE)
    src_guide["material"] = [[0, 3], [0, 3]]                               # left column sky, right column a kind-0 hit of material 3
    src = np.zeros((2, 2, 4), F)
    src[:, 0], src[:, 1] = F(1), F(100)
    dst_guide = np.zeros((3, 3), GUIDE_DTYPE)
    dst_guide["material"] = [[0, 0, 3], [0, 3, 3], [0, 0, 3]]
    out, cls = model.upsample(dst_guide, src, src_guide)
    assert (cls == 1).all()
    assert (out[dst_guide["material"] == 0] == F(1)).all() and (out[dst_guide["material"] == 3] == F(100)).all()
