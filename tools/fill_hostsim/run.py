#!/usr/bin/env python3
"""csrc/tdt_fill.hip and the bit-volume unit it shares with exact distance, csrc/tdt_bitvol.hip — kernels and host code,
unchanged — compiled for the CPU and run against a plain BFS, under AddressSanitizer and UBSan.  No GPU, no HIP:
hip/hip_runtime.h here stands in for the constructs the units use (a block is 256
real threads behind a pthread barrier, blocks run one after another, hipMalloc is malloc), device_scan.hpp for the scan, and
main.cpp supplies the pieces of the sibling units the unit calls (the tree's voxel list, the sort) and the cases: random grids
at depth 3-5 under both connectivities with fixed and inherited materials, the solid form, boxes whose walls straddle words of
a row at depth 7, one of them opened, the thin boxes that skip the flood.  A stand-alone program: nothing of it is loaded into
python or linked into libtdtrt.so.

    python tools/fill_hostsim/run.py [case-file]     # case-file: "depth conn material solid" then "x y z m" per wall voxel"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "tdt4230_project_raytracing_amd", "csrc")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        # the unit is compiled from a copy next to the stand-in headers, so that its quoted includes find those first
        shutil.copy(os.path.join(CSRC, "tdt_fill.hip"), os.path.join(tmp, "fill_unit.cpp"))
        shutil.copy(os.path.join(CSRC, "tdt_bitvol.hip"), os.path.join(tmp, "bitvol_unit.cpp"))
        for f in ("region_device.hpp", "bitvol_device.hpp"):
            shutil.copy(os.path.join(CSRC, f), tmp)
        for f in ("device_scan.hpp", "main.cpp"):
            shutil.copy(os.path.join(HERE, f), tmp)
        exe = os.path.join(tmp, "fill_hostsim")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                        "-I", tmp, "-I", HERE, "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++",
                        os.path.join(tmp, "fill_unit.cpp"), os.path.join(tmp, "bitvol_unit.cpp"), os.path.join(tmp, "main.cpp"), "-o", exe], check=True)
        return subprocess.run([exe] + sys.argv[1:]).returncode


if __name__ == "__main__":
    sys.exit(main())
