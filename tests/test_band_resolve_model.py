"""The rule the five-wave whole-depth builds serve a lane in a band by (csrc/trace_device.hpp band_classify, band_resolve_x), in numpy
float32 (tests/band_resolve_model.py) against the level walk, on the depth-5 tree of test_gpu_full_grid_corners:

  2^D x above the integer n > 0   the walk ends where the plain-digit descent of position n or of n - 2^j ends (j = trailing zeros of
                                  n), chosen by the one decision a = fl(v + f) - v > 0.5 of the critical level D - j on the cell index
                                  the plain descent holds above it
  above 0, below an odd n         position floor(2^D x)
  below an even n, exactly n      left to the walk

Every float of every band of n = 1 .. 2^D (n = 0: the ends of every binade), on the two chain columns and 62 drawn ones; the device
check (tdt_selftest 19, tests/test_gpu_band_resolve.py) runs every column."""
import numpy as np
import pytest

import band_resolve_model as model
import test_gpu_full_grid_corners as corners

DEPTH = 5
F = np.float32


@pytest.fixture(scope="module")
def cells():
    return corners._tree(DEPTH)


def _columns():
    side = 1 << DEPTH
    rng = np.random.default_rng(19)
    idx = rng.permutation(side * side)[:62]
    return np.concatenate([[0, side - 1], idx // side]), np.concatenate([[0, side - 1], idx % side])


def _check(cells, x):
    yi, zi = _columns()
    x, yi, zi = x[:, None], yi[None, :], zi[None, :]
    kind, n, xg, a = model.resolve(cells, DEPTH, x, yi, zi)
    served = xg >= 0
    got = model.plain(cells, DEPTH, np.where(served, xg, 0), yi, zi)[:4]
    want = model.walk(cells, DEPTH, x, yi, zi)
    same = np.ones(served.shape, bool)
    for g, w in zip(got, want):
        same &= g == w
    bad = served & ~same
    assert not bad.any(), f"{int(bad.sum())} lanes, first x = {float(np.broadcast_to(x, bad.shape)[bad][0])!r}"
    return kind, n, xg, a


def test_every_float_of_every_band(cells):
    seen = {model.FLOOR: 0, model.PARENT_IDX: 0, model.WALK: 0}
    a_seen = set()
    for n in range(1, (1 << DEPTH) + 1):
        x = model.band_floats(DEPTH, n)
        assert model.in_band(x, DEPTH).all() and len(x) >= 2 * 128
        kind, _, xg, a = _check(cells, x)
        for k in seen:
            seen[k] += int((kind == k).sum())
        a_seen |= set(np.unique(a[a >= 0]).tolist())
        # below an even n and on n itself: the walk's; everything else is served
        tg = (x * F(1 << DEPTH))[:, None]
        keep = (tg == n) | ((tg < n) & (n % 2 == 0))
        assert ((xg < 0) == np.broadcast_to(keep, xg.shape)).all()
    assert all(seen.values()) and a_seen == {0, 1}, (seen, a_seen)


def test_the_band_of_zero(cells):
    top = int(np.array(model.BAND / F(1 << DEPTH), F).view(np.uint32))
    bits = np.array([(e << 23) | m for e in range((top >> 23) + 1) for m in list(range(32)) + list(range(0x7FFFE0, 0x800000))], np.uint32)
    x = bits[(bits > 0) & (bits <= top)].view(F)
    assert model.in_band(x, DEPTH).all()
    kind, n, xg, _ = _check(cells, x)
    assert (kind == model.FLOOR).all() and (n == 0).all() and (xg == 0).all()
    # +0 itself is a tie
    assert model.classify(F(0.0), DEPTH)[0] == model.WALK


def test_both_positions_name_one_cell_when_the_descent_ends_above_the_critical_level(cells):
    """The parent-index table holds 0 where the plain descent ended before the critical level: that value is never decisive."""
    side = 1 << DEPTH
    yi, zi = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    ended = 0
    for n in range(1, side):
        j = int(model.trailing_zeros(n))
        hi, lo = model.plain(cells, DEPTH, n, yi, zi), model.plain(cells, DEPTH, n - (1 << j), yi, zi)
        early = hi[0] < DEPTH - j                                         # levels visited < lc
        ended += int(early.sum())
        for g, w in zip(hi[:4], lo[:4]):
            assert (g[early] == w[early]).all(), n
        assert (hi[4][DEPTH - 1 - j][early] == 0).all()                  # the index after lc - 1 levels, as the table stores it
    assert ended > 0
