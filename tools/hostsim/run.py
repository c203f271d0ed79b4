#!/usr/bin/env python3
"""A bit-volume unit (csrc/tdt_fill.hip, tdt_distance.hip, tdt_xform.hip, tdt_geodesic.hip or tdt_smooth.hip) and the layers under it
(csrc/tdt_bitvol.hip, bitvol_device.hpp; the capped tree list of csrc/tdt_voxlist.hip) — kernels and host code, unchanged — compiled for the CPU and run against a brute-force
model, under AddressSanitizer and UBSan.  No GPU, no HIP: hip/hip_runtime.h here stands in for the constructs the units use (a
block is 256 real threads behind a pthread barrier, blocks run one after another, hipMalloc is malloc), device_scan.hpp for the
scan, siblings.hpp for the pieces of the sibling units a unit calls (the slot check, the tree's voxel list, the sort, the edit
that takes the list) and for what the models share; <unit>.cpp holds the unit's model and its cases, hand-picked and small
because every block costs 256 threads:

    fill      a plain BFS: random grids at depth 3-5 under both connectivities with fixed and inherited materials, the solid
              form, boxes whose walls straddle words of a row at depth 7, one of them opened, the thin boxes that skip the flood
    distance  an all-pairs brute force and the ops' definitions: a sparse and a dense random grid at depth 3 and 4 cover the five
              ops, both borders, fixed and inherited materials and a box + sphere mask; pairs across a word boundary at depth 6
              (an axis tie, a diagonal tie); a full and an empty grid; depth 1 with R = 64; the field with its nearest voxels
    xform     a brute force over every destination voxel, dividing in 128-bit integers with an explicit floor where the unit
              shifts: identity, translations (one by -N + 1, one across a word boundary), quarter turns with even and odd pivots,
              a mirror with a fixed material, x2, x1/2, 3/2 with a destination box that cuts through bricks, a 30 degree rotation
              under a mask, entries of +-2^20, an offset of 2^40, an empty mask, an empty tree
    geodesic  a heap Dijkstra on a dense grid: random grids in both media with the weights {1,0,0}, {1,1,1}, {3,4,5}, {2,3,0},
              {5,1,1}, {7,0,2}, a material match, a mask, max_cost 0 and cuts, seeds off the grid and off the medium, no seeds,
              an empty mask, the empty tree, a serpentine corridor that needs more than one batch of passes, a corridor across a
              word boundary; each compares the field, the list, the list the edit form hands on and the canonical path
    smooth    a brute force over every offset of the ball: random grids at depth 3 and 4 under majority and Q16 thresholds, the
              three modes, both borders, fixed and inherited materials, a box + sphere mask and up to three iterations; radius2
              225 on a grid smaller than the ball; a tied pair and a bar across the words of a row at depth 6; a full grid, an
              empty one and a single voxel; the density field with its support.  The edit form's list is what it hands the builder

A stand-alone program: nothing of it is loaded into python or linked into libtdtrt.so.

    python tools/hostsim/run.py <unit> [case-file]    # fill only: "depth conn material solid" then "x y z m" per wall voxel"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "tdt4230_project_raytracing_amd", "csrc")
UNITS = ("fill", "distance", "xform", "geodesic", "smooth")


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in UNITS:
        sys.exit("usage: run.py {" + ",".join(UNITS) + "} [case-file]")
    unit = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        # the units are compiled from copies next to the stand-in headers, so that their quoted includes find those first
        srcs = [os.path.join(tmp, unit + "_unit.cpp"), os.path.join(tmp, "bitvol_unit.cpp"), os.path.join(tmp, "voxlist_unit.cpp"),
                os.path.join(tmp, unit + ".cpp")]
        for src, name in zip(srcs, ("tdt_" + unit + ".hip", "tdt_bitvol.hip", "tdt_voxlist.hip")):
            shutil.copy(os.path.join(CSRC, name), src)
        for f in ("region_device.hpp", "bitvol_device.hpp"):
            shutil.copy(os.path.join(CSRC, f), tmp)
        for f in ("device_scan.hpp", "siblings.hpp", unit + ".cpp"):
            shutil.copy(os.path.join(HERE, f), tmp)
        exe = os.path.join(tmp, unit + "_hostsim")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                        "-I", tmp, "-I", HERE, "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++"] + srcs + ["-o", exe], check=True)
        return subprocess.run([exe] + sys.argv[2:]).returncode


if __name__ == "__main__":
    sys.exit(main())
