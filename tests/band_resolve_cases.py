"""The frames of tests/test_gpu_band_resolve.py and of its child process (band_resolve_stats_frames.py): plane bundles with d_x = +0
whose plane lies m ulps beside the grid plane k of 2^depth — every sample point of every primary ray has the one local x coordinate
lx = k / 2^depth +- m ulp(lx), which is inside the band of k and off the plane.  Plain numpy: no GPU."""
import numpy as np

import band_resolve_model as model
import degenerate_cams

F = np.float32
W, H, SPP, BOUNCE = 96, 64, 4, 4
OFFSETS = (1, 3, 16, 60, 120)                  # m
CORNER_X = F(-0.5)                             # the reference corner


def grid_planes(depth):
    """{kind: k}: odd, 2 mod 4, and 2^(depth - 1) (critical level 1), all with k / 2^depth in [0.25, 0.75]."""
    half = 1 << (depth - 1)
    return {"odd": half - 5, "two_mod_four": half + 6, "half": half}


def cases(depth):
    """[(name, k, signed m)]"""
    return [(f"{kind}-{'above' if s > 0 else 'below'}-{m}", k, s * m) for kind, k in grid_planes(depth).items() for s in (1, -1) for m in OFFSETS]


def local_x(depth, k, m):
    """k / 2^depth moved by m ulps of itself (m < 0: below), as a float32."""
    lx = F(k) / F(1 << depth)
    assert 0.25 <= float(lx) <= 0.75 and float(lx) * (1 << depth) == k
    ulp = np.spacing(lx)                          # (lx is not a power of two except 0.5, whose lower neighbours are half as far: below 0.5 use that)
    if m < 0 and float(lx) == 0.5:
        ulp = ulp / F(2)
    out = F(lx + F(m) * ulp)
    assert float(out) == float(lx) + m * float(ulp)
    return out


def side(depth, k, m):
    """What band_classify makes of the case, from the kernel's own float32 expressions: "above", "odd_below" or "even_below"."""
    lx = local_x(depth, k, m)
    tg = F(lx * F(1 << depth))
    rn = np.rint(tg)
    assert int(rn) == k and bool(model.in_band(lx, depth)) and tg != rn, (depth, k, m)
    if tg > rn:
        assert m > 0
        return "above"
    assert m < 0
    return "odd_below" if k & 1 else "even_below"


def camera(depth, k, m):
    lx = local_x(depth, k, m)
    ox = F(lx + CORNER_X)                         # lx - 0.5
    assert float(ox) == float(lx) - 0.5 and F(ox + -CORNER_X) == lx      # both exact: the step's lx = w_x + -min_x is this lx
    cam = degenerate_cams.plane_bundle(0, (ox, -0.1, -0.3), w=W, h=H, spp=SPP, bounce=BOUNCE)
    assert degenerate_cams.axis_component_bits(cam, 0) == [0]             # d_x = +0 for every pixel and sample
    return cam
