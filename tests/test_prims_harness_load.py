"""The test-only harness over the device scan and radix sort (libtdtprims_selftest.so) is built with the other libraries,
loads on a machine without a GPU, exports its entry points and, like the product, reports a missing device as an error."""
import ctypes

import numpy as np

import prims_harness as ph
from tdt4230_project_raytracing_amd import rt


def test_harness_library_loads_and_exports_its_entry_points():
    L = ph.lib()
    for name in ("selftest_scan_u32", "selftest_sort_pairs_u32", "selftest_guard_report_words", "selftest_front_words", "selftest_canary"):
        assert hasattr(L, name), f"libtdtprims_selftest.so does not export {name}"
    want = ph.expected_report()
    guard = want[L.selftest_front_words():]
    assert guard.size >= 64 and len(set(guard.tolist())) == guard.size


def test_harness_is_not_part_of_the_product_library():
    L = ctypes.CDLL(rt.LIB_PATH)
    assert not hasattr(L, "selftest_scan_u32") and not hasattr(L, "selftest_sort_pairs_u32")
    assert not any(name.startswith("selftest") for name, _, _ in rt.SYMBOLS)


def test_status_says_whether_there_was_a_device():
    import torch
    have = torch.cuda.is_available()
    a = np.arange(5000, dtype=np.uint32)
    st, out, _, _ = ph.scan_raw(a)
    assert (st == 0) == have, f"selftest_scan_u32 returned {st}"
    st2, keys, vals, _ = ph.sort_raw(a[::-1].copy(), a)
    assert (st2 == 0) == have, f"selftest_sort_pairs_u32 returned {st2}"
    if have:
        assert (out == (np.cumsum(a, dtype=np.uint64) - a).astype(np.uint32)).all()
        assert (keys == a).all() and (vals == a[::-1]).all()
