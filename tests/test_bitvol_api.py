"""The dense bit-volume layer that four units share — enclosed space, exact distance, affine transforms and geodesic distance
(csrc/tdt_bitvol.hip, csrc/bitvol_device.hpp) — without a GPU: its three kernels cross-compile without scratch or spills, and what
the editing units used to keep a copy of each — the layer's pieces, from the tree's list to the result's, and the host helpers of
tdt_internal.hpp / region_device.hpp — has exactly one definition under csrc/."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tdt4230_project_raytracing_amd", "csrc")


def test_bitvol_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_bitvol.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert names == {"bitvol_bbox_kernel", "bitvol_rasterise_kernel", "bitvol_list_kernel"}
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


# what is matched is the DEFINITION (its characteristic line), not the name: a copy under another name is found too
ONE_DEFINITION = {
    "the valid-bits mask": (r"m &= 0xFFFFFFFFu >> \(31 - \(B\.hi\[0\] & 31\)\)", "bitvol_device.hpp"),
    "the box struct": (r"int32_t nw, wx0;", "bitvol_device.hpp"),
    "the bounding-box kernel": (r"atomicMax\(box \+ 3 \+ a, h\)", "tdt_bitvol.hip"),
    "the rasterise kernel": (r"atomicOr\(occ \+ row \* \(uint32_t\)B\.nw", "tdt_bitvol.hip"),
    "the list kernel": (r"out\[i\] = make_int4\(\(int\)region_compact3\(k >> 2\)", "tdt_bitvol.hip"),
    "the sorted-key lookup": (r"if \(keys\[mid\] <= k\) lo = mid; else hi = mid;", "bitvol_device.hpp"),
    "blocks_of": (r"\(lanes \+ 255\) / 256", "tdt_internal.hpp"),
    "the drain guard": (r"~\w+\(\) \{ \(void\)hipStreamSynchronize\(", "tdt_internal.hpp"),
    "the shape check": (r"shape must be TDT_SHAPE_BOX", "region_device.hpp"),
    "the list tail's total read": (r"hipMemcpyAsync\(&\w+, count \+ ", "bitvol_device.hpp"),
    "the pass loop's last-flag test": (r"while \(h_flags\[k\w+ - 1\]\)", "bitvol_device.hpp"),
    # (tdt_morph.hip and tdt_surface.hip, voxel-list units outside the layer, hold the same text against caps of their own)
    "the tree cap": (r"k(Fill|Dist|Xform|Geo|Bitvol)Cap\b.*\"the tree holds \"", "tdt_bitvol.hip"),
    "the field box": (r"\"the box holds \"", "bitvol_device.hpp"),
    "the extract frame": (r"list_to_host\(ctx, m->stream, vox, n, sizeof\(int4\), \"voxels\"", "tdt_internal.hpp"),
}


@pytest.mark.parametrize("what", list(ONE_DEFINITION))
def test_shared_piece_has_one_definition(what):
    pattern, owner = ONE_DEFINITION[what]
    owners = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".h", ".cpp")) and re.search(pattern, open(os.path.join(CSRC, f)).read())]
    assert owners == [owner]
