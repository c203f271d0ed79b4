"""The two layers under the editing units, without a GPU: the dense bit volume that four units share — enclosed space, exact
distance, affine transforms and geodesic distance (csrc/tdt_bitvol.hip, csrc/bitvol_device.hpp) — and the Morton-sorted voxel list
every list-based unit starts from (csrc/tdt_voxlist.hip).  Their kernels cross-compile without scratch or spills, and what the
editing units used to keep a copy of each — the bit volume's pieces, from the tree's list to the result's; the list layer's
kernels and frames; the device helpers of region_device.hpp (searches, the key's voxel, Morton arithmetic) and the host helpers
of tdt_internal.hpp (first member, the replicas' edit frame, the rebuild tail, the word read) — has exactly one definition under
csrc/."""
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


def test_voxlist_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_voxlist.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {n for n in names if not n.startswith("scan_")} == {"voxlist_keys_kernel", "voxlist_last_flags_kernel", "voxlist_unique_kernel",
                                                               "voxlist_gather_kernel"}       # (scan_*: device_scan.hpp's, in every unit)
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


# what is matched is the DEFINITION (its characteristic line), not the name: a copy under another name is found too
ONE_DEFINITION = {
    "the valid-bits mask": (r"m &= 0xFFFFFFFFu >> \(31 - \(B\.hi\[0\] & 31\)\)", "bitvol_device.hpp"),
    "the box struct": (r"int32_t nw, wx0;", "bitvol_device.hpp"),
    "the bounding-box kernel": (r"atomicMax\(box \+ 3 \+ a, h\)", "tdt_bitvol.hip"),
    "the rasterise kernel": (r"atomicOr\(occ \+ row \* \(uint32_t\)B\.nw", "tdt_bitvol.hip"),
    "the list kernel": (r"out\[i\] = region_voxel\(keys\[i\], \(int\)vals\[i\]\)", "tdt_bitvol.hip"),
    "the sorted-key lookup": (r"if \(keys\[mid\] <= k\) lo = mid; else hi = mid;", "bitvol_device.hpp"),
    "blocks_of": (r"\(lanes \+ 255\) / 256", "tdt_internal.hpp"),
    "the drain guard": (r"~\w+\(\) \{ \(void\)hipStreamSynchronize\(", "tdt_internal.hpp"),
    "the shape check": (r"shape must be TDT_SHAPE_BOX", "region_device.hpp"),
    "the list tail's total read": (r"read_word\(front, st, count \+ n_items, &\w+\)", "bitvol_device.hpp"),
    "the pass loop's last-flag test": (r"while \(h_flags\[k\w+ - 1\]\)", "bitvol_device.hpp"),
    "the tree cap": (r"k(Fill|Dist|Xform|Geo|Bitvol|Morph|Surface|VoxelList)Cap\b.*\"the tree holds \"", "tdt_voxlist.hip"),
    "the field box": (r"\"the box holds \"", "bitvol_device.hpp"),
    "the extract frame": (r"list_to_host\(ctx, m->stream, vox, n, sizeof\(int4\), \"voxels\"", "tdt_internal.hpp"),
    # ---- the voxel-list layer (tdt_voxlist.hip) and the helpers under it ----
    "the first-member ternary": (r"->multi \? (tdt::)?multi_first_member\(", "tdt_internal.hpp", {"tdt_rt.hip"}),   # (the trace unit keeps its own)
    "the slot text": (r"\"no buffer bound to shader-storage slot \"\)", "tdt_internal.hpp"),
    "the rebuild tail's error forward": (r"return ctx == front \? rc : fail\(front, rc, tdt_last_error\(ctx\)\)", "tdt_internal.hpp"),
    # a copy of ONE 32-bit word to the host with the synchronisation right behind it (the 64-bit totals and the multi-word reads stay)
    "the word read": (r"hipMemcpyAsync\(&?\w+, [^,;]+, sizeof ?\(?(uint32_t|n\w*)\)?, hipMemcpyDeviceToHost, \w+\)\);[^\n]*\n\s*TDT_HIP\(\w+, hipStreamSynchronize",
                      "tdt_internal.hpp"),
    "the keys kernel": (r"\w+\[i\] = region_key\(p\.x, p\.y, p\.z\); \}", "tdt_voxlist.hip"),
    "the last-of-run flags": (r"keys\[i\] != k\w*Dropped\w* && \(i \+ 1u == n \|\| keys\[i \+ 1u\] != keys\[i\]\)", "tdt_voxlist.hip"),
    "the (key, value) unique": (r"if \(i == 0\) \*count = excl\[n\];", "tdt_voxlist.hip"),
    "the gather": (r"\bo\w*\[excl\[i\]\] = \w+\[i\];", "tdt_voxlist.hip"),
    "the lower-bound loop": (r"\[mid\] < \w+\) lo = mid \+ 1; else hi = mid;", "region_device.hpp"),
    "the upper-bound loop": (r"\[mid\] <= \w+\) lo = mid \+ 1; else hi = mid;", "region_device.hpp"),
    "the key's voxel": (r"make_int4\(\(int\)\w*compact3\(\w+ >> 2\)", "region_device.hpp"),
    "spread3": (r"\(v \| \(v << 16\)\) & 0x030000FFu", "region_device.hpp"),
    "compact3": (r"v &= 0x09249249u;", "region_device.hpp"),
}


@pytest.mark.parametrize("what", list(ONE_DEFINITION))
def test_shared_piece_has_one_definition(what):
    pattern, owner, *apart = ONE_DEFINITION[what]                  # apart: files out of the layers' scope that are known to hold a copy
    owners = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".h", ".cpp")) and f not in set().union(*apart)
              and re.search(pattern, open(os.path.join(CSRC, f)).read())]
    assert owners == [owner]
