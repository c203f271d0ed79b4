#!/usr/bin/env python3
"""csrc/tdt_xform.hip and the bit-volume unit it uses, csrc/tdt_bitvol.hip — kernels and host code, unchanged — compiled for the
CPU and run against a brute force over every destination voxel, under AddressSanitizer and UBSan.  No GPU, no HIP:
hip/hip_runtime.h here (on top of tools/distance_hostsim's and tools/fill_hostsim's) stands in for the constructs the unit uses,
tools/fill_hostsim/device_scan.hpp for the scan, and main.cpp supplies the pieces of the sibling units the unit calls (the tree's
voxel list, the sort, the edit that takes the list) and the cases, about fifteen, hand-picked because a block is 256 real threads:
identity, translations (one by -N + 1, one across a word boundary at depth 6), quarter turns with even and odd pivots, a mirror
with a fixed material, x2, x1/2 and 3/2 with a destination box that cuts through bricks, a 30 degree rotation under a box +
sphere mask, entries of +-2^20, an offset of 2^40, an empty mask and an empty tree.  The brute force
divides in 128-bit integers with an explicit floor where the unit shifts.  A stand-alone program: nothing of it is loaded into
python or linked into libtdtrt.so.

    python tools/xform_hostsim/run.py"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "tdt4230_project_raytracing_amd", "csrc")
FILL = os.path.join(os.path.dirname(HERE), "fill_hostsim")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        # the unit is compiled from a copy next to the stand-in headers, so that its quoted includes find those first
        shutil.copy(os.path.join(CSRC, "tdt_xform.hip"), os.path.join(tmp, "xform_unit.cpp"))
        shutil.copy(os.path.join(CSRC, "tdt_bitvol.hip"), os.path.join(tmp, "bitvol_unit.cpp"))
        for f in ("region_device.hpp", "bitvol_device.hpp"):
            shutil.copy(os.path.join(CSRC, f), tmp)
        shutil.copy(os.path.join(FILL, "device_scan.hpp"), tmp)
        shutil.copy(os.path.join(HERE, "main.cpp"), tmp)
        exe = os.path.join(tmp, "xform_hostsim")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                        "-I", tmp, "-I", HERE, "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++",
                        os.path.join(tmp, "xform_unit.cpp"), os.path.join(tmp, "bitvol_unit.cpp"), os.path.join(tmp, "main.cpp"), "-o", exe], check=True)
        return subprocess.run([exe] + sys.argv[1:]).returncode


if __name__ == "__main__":
    sys.exit(main())
