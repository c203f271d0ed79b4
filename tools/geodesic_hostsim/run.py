#!/usr/bin/env python3
"""csrc/tdt_geodesic.hip and the bit-volume unit it uses, csrc/tdt_bitvol.hip — kernels and host code, unchanged — compiled for
the CPU and run against a brute-force Dijkstra on a dense grid, under AddressSanitizer and UBSan.  No GPU, no HIP:
hip/hip_runtime.h here (tools/xform_hostsim's, on top of tools/distance_hostsim's and tools/fill_hostsim's) stands in for the
constructs the unit uses, tools/fill_hostsim/device_scan.hpp for the scan, and main.cpp supplies the pieces of the sibling units
the unit calls (the tree's voxel list, the sort, the edit that takes the list) and the cases, fifteen, small because a block is
256 real threads: random grids in both media with the weights {1,0,0}, {1,1,1}, {3,4,5}, {2,3,0}, {5,1,1}, {7,0,2}, a material
match, a box + sphere mask, max_cost 0 and cuts, seeds off the grid and off the medium, no seeds, an empty mask, the empty tree in
both media, a serpentine corridor that needs more than one batch of passes (whole and cut mid-way), and a corridor across a word
boundary with a seed at either end.  Every case compares the field, the list, the list the edit form hands on and the canonical
path.  A stand-alone program: nothing of it is loaded into python or linked into libtdtrt.so.

    python tools/geodesic_hostsim/run.py"""
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
        shutil.copy(os.path.join(CSRC, "tdt_geodesic.hip"), os.path.join(tmp, "geodesic_unit.cpp"))
        shutil.copy(os.path.join(CSRC, "tdt_bitvol.hip"), os.path.join(tmp, "bitvol_unit.cpp"))
        for f in ("region_device.hpp", "bitvol_device.hpp"):
            shutil.copy(os.path.join(CSRC, f), tmp)
        shutil.copy(os.path.join(FILL, "device_scan.hpp"), tmp)
        shutil.copy(os.path.join(HERE, "main.cpp"), tmp)
        exe = os.path.join(tmp, "geodesic_hostsim")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                        "-I", tmp, "-I", HERE, "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++",
                        os.path.join(tmp, "geodesic_unit.cpp"), os.path.join(tmp, "bitvol_unit.cpp"), os.path.join(tmp, "main.cpp"), "-o", exe], check=True)
        return subprocess.run([exe] + sys.argv[1:]).returncode


if __name__ == "__main__":
    sys.exit(main())
