"""Resource gate of the five-wave whole-depth builds (CPU: hipcc cross-compiles): five 256-thread blocks share a CU only if each
stays within 96 VGPRs and 32 KiB of LDS, and a build that spills to get there is slower than the four-wave one it replaces.  The
compiler's own table (tools/kernel_resources.py), not the attribute that asks for the occupancy.  Every other build keeps the limits
of its 1024-thread block."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _args(row):
    return [a.strip() for a in row["name"][len("tdt::trace_kernel<"):-1].split(",")]


def _five(row):
    a = _args(row)
    return len(a) >= 10 and a[8] == "256" and a[9] == "5"


@pytest.fixture(scope="module")
def rows():
    import kernel_resources
    return [r for r in kernel_resources.collect() if r["name"].startswith("tdt::trace_kernel<false")]


def test_five_wave_builds_fit_five_blocks_per_cu(rows):
    five = [r for r in rows if _five(r)]
    # depth 5 / 6 x the UNIT / multiplying build: whole-depth (FULL), resident, not BRICK
    assert sorted((a[2], a[6]) for a in map(_args, five)) == [("5", "false"), ("5", "true"), ("6", "false"), ("6", "true")]
    for r in five:
        a = _args(r)
        assert a[1] == "1" and a[3] == "true" and a[5] == "true" and a[7] == "false", r
        assert r["VGPRs"] <= 96, r
        assert r["AGPRs"] == 0, r
        assert r["ScratchSize [bytes/lane]"] == 0, r
        assert r["VGPRs Spill"] == 0, r
        assert r["Occupancy [waves/SIMD]"] == 5, r
        assert r["LDS Size [bytes/block]"] <= 32768, r
        assert r["SGPRs Spill"] <= 44, r              # (tests/test_kernel_resources.py: the ceiling of the builds that are not BRICK)


def test_every_other_build_keeps_its_limits(rows):
    others = [r for r in rows if not _five(r)]
    assert len(others) >= 68                          # kTraceVariants' 1024 x 1 rows (the four-wave whole-depth builds among them) + the two general kernels
    for r in others:
        assert r["ScratchSize [bytes/lane]"] == 0, r
        assert r["VGPRs Spill"] == 0, r
        assert r["Occupancy [waves/SIMD]"] >= 4, r
        assert r["VGPRs"] <= 128, r
        assert r["LDS Size [bytes/block]"] <= 160 * 1024, r
        a = _args(r)
        if len(a) >= 3 and a[2] != "0":               # (tests/test_kernel_resources.py: the general kernels are exempt)
            assert r["SGPRs Spill"] <= (8 if a[7] == "true" else 44), r
