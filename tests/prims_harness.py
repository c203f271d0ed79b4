"""ctypes wrapper over libtdtprims_selftest.so (csrc/prims_selftest.hip): the device scan and the radix sort run on host
arrays, every device array canary-guarded.  Test-only; the package does not know this library."""
import ctypes
import os

import numpy as np

from tdt4230_project_raytracing_amd import rt

# TDT_SELFTEST_LIB: another build of the harness, as TDT_LIB is another build of libtdtrt.so (A/B runs)
LIB_PATH = os.environ.get("TDT_SELFTEST_LIB") or os.path.join(os.path.dirname(os.path.abspath(rt.__file__)), "libtdtprims_selftest.so")
SCAN_ARRAYS = ("in", "out", "scratch")
SORT_ARRAYS = ("keys0", "keys1", "vals0", "vals1", "hist", "scratch")

_lib = None
_u32p = ctypes.POINTER(ctypes.c_uint32)


class HarnessError(RuntimeError):
    def __init__(self, what, status):
        super().__init__(f"{what}: hipError_t {status}")
        self.status = status


def lib():
    global _lib
    if _lib is None:
        rt.lib()                                             # torch's HIP runtime first, and libtdtrt.so itself (see rt.lib)
        L = ctypes.CDLL(LIB_PATH)
        for f in (L.selftest_guard_report_words, L.selftest_front_words):
            f.restype, f.argtypes = ctypes.c_uint32, []
        L.selftest_canary.restype = ctypes.c_uint32
        L.selftest_canary.argtypes = [ctypes.c_uint32]
        L.selftest_scan_u32.restype = ctypes.c_int
        L.selftest_scan_u32.argtypes = [_u32p, _u32p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                        _u32p, _u32p]
        L.selftest_sort_pairs_u32.restype = ctypes.c_int
        L.selftest_sort_pairs_u32.argtypes = [_u32p, _u32p, ctypes.c_uint32, _u32p, _u32p, _u32p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(_u32p)


def _u32(a):
    return np.ascontiguousarray(a, np.uint32).reshape(-1)


def expected_report():
    """What one array's canary report holds when nothing wrote outside the payload: front words, then guard words."""
    L = lib()
    front = L.selftest_front_words()
    return np.array([L.selftest_canary(j) for j in range(front)] +
                    [L.selftest_canary(j) for j in range(L.selftest_guard_report_words() - front)], np.uint32)


def scan_raw(a, in_place=False, skew_in=0, skew_out=0, skew_scratch=0):
    """(status, out, in_after, {array name: canary report}) of one exclusive_scan_u32 over `a` on the device."""
    L = lib()
    a = _u32(a)
    out, after = np.zeros(a.size, np.uint32), np.zeros(a.size, np.uint32)
    guards = np.zeros((len(SCAN_ARRAYS), L.selftest_guard_report_words()), np.uint32)
    st = L.selftest_scan_u32(_p(a), _p(out), a.size, int(in_place), skew_in, skew_out, skew_scratch, _p(after), _p(guards))
    return st, out, after, dict(zip(SCAN_ARRAYS, guards))


def scan(a, **kw):
    st, out, after, guards = scan_raw(a, **kw)
    if st != 0:
        raise HarnessError("selftest_scan_u32", st)
    return out, after, guards


def sort_raw(keys, vals):
    """(status, sorted keys, sorted values, {array name: canary report}) of one tdt::sort_pairs_u32 on the device."""
    L = lib()
    keys, vals = _u32(keys), _u32(vals)
    assert keys.size == vals.size
    ko, vo = np.zeros(keys.size, np.uint32), np.zeros(keys.size, np.uint32)
    guards = np.zeros((len(SORT_ARRAYS), L.selftest_guard_report_words()), np.uint32)
    st = L.selftest_sort_pairs_u32(_p(keys), _p(vals), keys.size, _p(ko), _p(vo), _p(guards))
    return st, ko, vo, dict(zip(SORT_ARRAYS, guards))


def sort_pairs(keys, vals):
    st, ko, vo, guards = sort_raw(keys, vals)
    if st != 0:
        raise HarnessError("selftest_sort_pairs_u32", st)
    return ko, vo, guards


def where(i, sort=False):
    """Which stage of a 2048-item tile index i belongs to.  The scan gives a lane 8 consecutive items (4 waves x 64 lanes
    x 8); the sort walks a tile in 8 rounds of 256 consecutive items, one per lane."""
    i = int(i)
    s = f"index {i}: tile {i // 2048}, wave {(i % 2048) // 512}, lane {(i % 512) // 8}, item {i % 8}"
    if sort:
        s += f" (sort layout: round {(i % 2048) // 256}, wave {(i % 256) // 64}, lane {i % 64})"
    return s


def assert_equal_u32(got, want, what, sort=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint32 and want.dtype == np.uint32 and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ, first at {where(bad[0], sort)}: "
                           f"got {int(got[bad[0]])}, want {int(want[bad[0]])}")


def assert_guards(guards, what):
    want = expected_report()
    for name, rep in guards.items():
        bad = np.flatnonzero(rep != want)
        front = lib().selftest_front_words()
        assert bad.size == 0, (f"{what}: out-of-bounds write next to `{name}`: "
                               + ", ".join(f"{'front' if j < front else 'guard'} word {j if j < front else j - front} = {int(rep[j]):#x}"
                                           for j in bad[:8]))
