#!/usr/bin/env python3
"""csrc/tdt_distance.hip and the bit-volume unit it shares with enclosed space, csrc/tdt_bitvol.hip — kernels and host code,
unchanged — compiled for the CPU and run against an all-pairs brute force and the ops' definitions, under AddressSanitizer and
UBSan.  No GPU, no HIP: hip/hip_runtime.h here (on top of tools/fill_hostsim's)
stands in for the constructs the unit uses, tools/fill_hostsim/device_scan.hpp for the scan, and main.cpp supplies the pieces of
the sibling units the unit calls (the slot check, the tree's voxel list, the sort, the edit that takes the delta list) and the
cases, about twenty, hand-picked because a block is 256 real threads and every case costs seconds: one sparse and one dense random
grid at depth 3 and at depth 4 between them cover the five ops, both borders, fixed and inherited materials and a box + sphere
mask; two pairs across a word boundary at depth 6 (an axis tie and a diagonal tie); a full and an empty grid; depth 1 with
R = 64; and the field with its nearest voxels on each of them.  A stand-alone program: nothing of it is
loaded into python or linked into libtdtrt.so.

    python tools/distance_hostsim/run.py"""
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
        shutil.copy(os.path.join(CSRC, "tdt_distance.hip"), os.path.join(tmp, "distance_unit.cpp"))
        shutil.copy(os.path.join(CSRC, "tdt_bitvol.hip"), os.path.join(tmp, "bitvol_unit.cpp"))
        for f in ("region_device.hpp", "bitvol_device.hpp"):
            shutil.copy(os.path.join(CSRC, f), tmp)
        shutil.copy(os.path.join(FILL, "device_scan.hpp"), tmp)
        shutil.copy(os.path.join(HERE, "main.cpp"), tmp)
        exe = os.path.join(tmp, "distance_hostsim")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                        "-I", tmp, "-I", HERE, "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++",
                        os.path.join(tmp, "distance_unit.cpp"), os.path.join(tmp, "bitvol_unit.cpp"), os.path.join(tmp, "main.cpp"), "-o", exe], check=True)
        return subprocess.run([exe] + sys.argv[1:]).returncode


if __name__ == "__main__":
    sys.exit(main())
