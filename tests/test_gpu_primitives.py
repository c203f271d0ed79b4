"""The two device primitives under every octree operation, tested on their own at the sizes where their code branches:
exclusive_scan_u32 (device_scan.hpp: 2048-item tiles, 8 items per lane, 4 waves, recursion on the tile sums, a 16-byte
vector load path and a scalar one) against numpy's cumsum, and tdt::sort_pairs_u32 (tdt_build.hip: 4 LSD passes of 8 bits
over 2048-item tiles walked in 8 rounds of 256 lanes) against numpy's stable argsort.  Integers only: every comparison is
exact.  The harness (csrc/prims_selftest.hip) gives the scratch arrays exactly the words the product's sizing functions
ask for and surrounds every device array with canaries, which every test asserts untouched."""
import functools
import zlib

import numpy as np
import pytest

import prims_harness as ph

pytestmark = pytest.mark.gpu

T = 2048
SCAN_SMALL = [1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, T * 5 + 3]
# two-level up to 2048^2, three-level above.  First-level tile counts: 2048, 2048, 2049, 2050 and 2052 — the third level's
# input is scratch + that count, so it is 16-byte aligned for the last size only.
SCAN_BIG = [T * T - 1, T * T, T * T + 1, T * T + T + 5, T * T + T * 3 + 5]
# 16 386 first-level tiles, 9 second-level ones: the only kind of size at which a lane of the THIRD level holds 8 whole
# items, so that the alignment test alone (scratch + 16 386 is 8 bytes off) keeps it away from the vector loads
SCAN_HUGE = 8 * T * T + T + 5
SCAN_PATTERNS = ("ones", "flags", "counts", "wrap", "one@0", "one@2047", "one@2048", "one@last")
SORT_SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 16384, 16385, T * 40 + 17]
SORT_PATTERNS = ("random32", "three_values", "all_equal", "ascending", "descending", "morton_dropped", "byte0", "byte1", "byte2",
                 "byte3", "tile_digit")
DROPPED = 0xFFFFFFFF


def _seed(*parts):
    return np.random.default_rng([zlib.crc32(str(p).encode()) for p in parts])


def scan_case(n, pattern):
    """(input, expected exclusive prefix sums mod 2^32), read-only, made once per (n, pattern); None: not applicable.
    The 16 MB-and-up cases are kept only while consecutive checks use them."""
    return (_scan_case_small if n <= 1 << 16 else _scan_case_big)(n, pattern)


def _scan_case(n, pattern):
    rng = _seed("scan", n, pattern)
    if pattern == "ones":
        a = np.ones(n, np.uint32)
    elif pattern == "flags":                                   # the callers' idiom: n - 1 flags and a 0, the total lands in out[n - 1]
        a = rng.integers(0, 2, size=n, dtype=np.uint32)
        a[-1] = 0
    elif pattern == "counts":                                  # morph's neighbour counts
        a = rng.integers(0, 27, size=n, dtype=np.uint32)
    elif pattern == "wrap":
        a = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    else:
        at = n - 1 if pattern == "one@last" else int(pattern[4:])
        if at >= n:
            return None
        a = np.zeros(n, np.uint32)
        a[at] = 1
    want = ((np.cumsum(a.astype(np.uint64)) - a) & 0xFFFFFFFF).astype(np.uint32)
    a.setflags(write=False)
    want.setflags(write=False)
    return a, want


_scan_case_small = functools.lru_cache(maxsize=None)(_scan_case)
_scan_case_big = functools.lru_cache(maxsize=2)(_scan_case)


def check_scan(n, pattern, in_place, **skews):
    case = scan_case(n, pattern)
    if case is None:
        return
    a, want = case
    what = f"scan n={n} {pattern} {'in place' if in_place else 'out of place'} {skews or ''}"
    out, after, guards = ph.scan(a, in_place=in_place, **skews)
    ph.assert_guards(guards, what)
    ph.assert_equal_u32(out, want, what)
    if not in_place:
        ph.assert_equal_u32(after, a, what + ": the input array was written")
    if pattern == "ones":
        assert out[-1] == (n - 1) & 0xFFFFFFFF
    if pattern == "flags":
        assert int(out[-1]) == int(a.sum(dtype=np.uint64)), what + ": out[n - 1] is not the number of flags"


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("n", SCAN_SMALL)
def test_scan_at_lane_wave_and_tile_edges(n, in_place):
    for pattern in SCAN_PATTERNS:
        check_scan(n, pattern, in_place)


@pytest.mark.parametrize("n", SCAN_BIG)
def test_scan_around_the_three_level_threshold(n):
    assert (n > T * T) == (-(-n // T) > T)                     # three levels exactly when the tile sums need tiles of their own
    for pattern, in_place in (("ones", False), ("flags", False), ("wrap", False), ("wrap", True), ("counts", True), ("one@last", False),
                              ("one@2048", True)):
        check_scan(n, pattern, in_place)


def test_scan_with_a_vector_width_third_level():
    check_scan(SCAN_HUGE, "counts", False)


SKEWS = [dict(skew_in=i, skew_out=o, skew_scratch=0) for i in range(4) for o in range(4)] + \
        [dict(skew_in=0, skew_out=0, skew_scratch=s) for s in (1, 2, 3)]


@pytest.mark.parametrize("n", [2049, T * T + T * 3 + 5])
def test_scan_with_misaligned_arrays(n):
    """A misaligned input takes the scalar loads at the top level; a misaligned scratch takes them one level down."""
    for pattern in (("flags", "wrap") if n < T * T else ("wrap",)):
        for skews in SKEWS:
            check_scan(n, pattern, False, **skews)
        for s in range(1, 4):                                  # in place: one array, so one skew
            check_scan(n, pattern, True, skew_out=s, skew_scratch=s)


@functools.lru_cache(maxsize=None)
def sort_case(n, pattern):
    """(keys, values = arange, expected keys, expected values) with numpy's stable argsort as the reference; read-only."""
    rng = _seed("sort", n, pattern)
    i = np.arange(n, dtype=np.uint64)
    if pattern == "random32":
        k = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    elif pattern == "three_values":                            # long runs of equal keys across lanes, waves, rounds and tiles
        k = np.array([0x00010203, 0xFFFFFFFF, 0x80000000], np.uint32)[rng.integers(0, 3, size=n)]
    elif pattern == "all_equal":
        k = np.full(n, 0x5A5A5A5A, np.uint32)
    elif pattern == "ascending":                               # spread over all four bytes
        k = (i * ((1 << 32) // n)).astype(np.uint32)
    elif pattern == "descending":
        k = (i * ((1 << 32) // n)).astype(np.uint32)[::-1].copy()
    elif pattern == "morton_dropped":                          # the builder: 30-bit keys, duplicates, ~5 % out-of-grid voxels
        k = rng.integers(0, 1 << 30, size=n, dtype=np.uint32)
        k[rng.integers(0, n, size=n // 3)] = k[rng.integers(0, n, size=n // 3)]
        k[rng.random(n) < 0.05] = DROPPED
    elif pattern.startswith("byte"):                           # one pass does all the work, the other three are pure stable copies
        k = (np.uint32(0x9C3A715E) & ~np.uint32(0xFF << (8 * int(pattern[4])))) | \
            (rng.integers(0, 256, size=n, dtype=np.uint32) << np.uint32(8 * int(pattern[4])))
    elif pattern == "tile_digit":                              # passes 1 and 3: a whole tile in one bin, each tile in another
        t = (i // T).astype(np.uint32)
        k = rng.integers(0, 1 << 32, size=n, dtype=np.uint32) & np.uint32(0x00FF00FF)
        k |= (((t * 7 + 3) & 255) << 8) | (((255 - t) & 255) << 24)
    k = k.astype(np.uint32)
    v = np.arange(n, dtype=np.uint32)
    o = np.argsort(k, kind="stable")
    out = (k, v, k[o], v[o])
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_is_stable_by_the_whole_key(n):
    for pattern in SORT_PATTERNS:
        k, v, want_k, want_v = sort_case(n, pattern)
        what = f"sort n={n} {pattern}"
        got_k, got_v, guards = ph.sort_pairs(k, v)
        ph.assert_guards(guards, what)
        ph.assert_equal_u32(got_k, want_k, what + " keys", sort=True)
        ph.assert_equal_u32(got_v, want_v, what + " values (equal keys must keep their order)", sort=True)
        if pattern == "morton_dropped":
            nd = int((k == DROPPED).sum())
            assert (got_k[n - nd:] == DROPPED).all() and (got_k[:n - nd] != DROPPED).all(), what + ": dropped keys must sort last"
