"""Region edits without a GPU: the entry points are exported and bound, the Python tdt_region layout is the header's, the
new kernels cross-compile without scratch or spills, and tdt_pick_grid_voxel lands on the cell tdt_pick_edit_delta aims at."""
import ctypes
import os
import re
import sys

import numpy as np

from tdt4230_project_raytracing_amd import host, rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_octree_edit_region", "tdt_octree_edit_voxels", "tdt_octree_extract_region")


def test_region_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    assert hasattr(host.lib(), "tdt_pick_grid_voxel")
    text = open(os.path.join(ROOT, "include", "tdt_host.h")).read()
    assert re.search(r"\bint tdt_pick_grid_voxel\s*\(", text)


def test_region_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_region \{(.*?)\} tdt_region;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\bint32_t\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert [f[0] for f in fields] == [f[0] for f in rt.Region._fields_]
    offset = 0
    for name, count in fields:
        assert getattr(rt.Region, name).offset == offset, name
        offset += 4 * (int(count) if count else 1)
    assert offset == ctypes.sizeof(rt.Region) == 32
    for name, value in (("TDT_SHAPE_BOX", rt.SHAPE_BOX), ("TDT_SHAPE_SPHERE", rt.SHAPE_SPHERE), ("TDT_REGION_SET", rt.REGION_SET),
                        ("TDT_REGION_FILL", rt.REGION_FILL), ("TDT_REGION_PAINT", rt.REGION_PAINT), ("TDT_REGION_CLEAR", rt.REGION_CLEAR)):
        assert re.search(rf"\b{name} = {value}\b", text), name
    assert re.search(r"#define TDT_REGION_BRUSH_CAP \(1u << 26\)", text) and rt.REGION_BRUSH_CAP == 1 << 26
    s = rt.sphere((-3, 4, 5), 7)
    assert (s.shape, list(s.a), list(s.b)) == (rt.SHAPE_SPHERE, [-3, 4, 5], [7, 0, 0])
    b = rt.box((1, 2, 3), (4, 5, 6))
    assert bytes(b) == np.array([0, 1, 2, 3, 4, 5, 6, 0], np.int32).tobytes()


def _hit(point, normal, status=None, fresh=1):
    rec = np.zeros(1, rt.RAY_HIT_DTYPE)
    rec["status"] = rt.RAY_HIT if status is None else status
    rec["fresh_record"] = fresh
    rec["point"] = point
    rec["normal"] = normal
    return rec[0]


def test_pick_grid_voxel_agrees_with_a_float64_model_and_the_edit_delta():
    rng = np.random.default_rng(4)
    for depth, min_point, scale in ((6, (-0.5, -0.5, -1.0), 1.0), (8, (-2.0, 0.25, 3.0), 2.5), (10, (0.0, 0.0, 0.0), 0.75)):
        floats = np.array([*min_point, 0.0, scale, 1.0 / scale, 1.0 / 1024], np.float32)
        ints = np.array([depth, 64, 1024], np.int32)
        cells = 1 << depth
        checked = 0
        for _ in range(300):
            axis, sign = int(rng.integers(3)), float(rng.choice([-1.0, 1.0]))
            k = rng.integers(0, cells, 3)
            u = (k + rng.uniform(0.05, 0.95, 3)) / cells
            u[axis] = (k[axis] + (1 if sign > 0 else 0)) / cells          # on a face of voxel k, facing out along `normal`
            normal = np.zeros(3, np.float32)
            normal[axis] = sign
            point = (np.float32(scale) * u.astype(np.float32) + floats[:3]).astype(np.float32)
            for place in (0, 1):
                q = (point.astype(np.float64) - floats[:3].astype(np.float64)) / np.float64(floats[4]) + \
                    (1.0 if place else -1.0) * normal.astype(np.float64) * (0.5 / cells)
                want = np.floor(q * cells)
                h = _hit(point, normal)
                if not ((want >= 0) & (want < cells)).all():
                    try:
                        host.pick_grid_voxel(h, (floats, ints), place)
                        raise AssertionError("expected a ValueError outside the grid")
                    except ValueError:
                        continue
                got = host.pick_grid_voxel(h, (floats, ints), place)
                assert got.dtype == np.int32 and list(got) == [int(v) for v in want]
                delta = host.pick_edit_delta(h, (floats, ints), place, 3.0)
                assert np.array_equal(delta[:3], ((got + 0.5) / cells).astype(np.float32))
                checked += 1
        assert checked > 400
    floats = np.array([0, 0, 0, 0, 1, 1, 1 / 1024], np.float32)
    ints = np.array([4, 64, 1024], np.int32)
    for bad in (_hit((0.5, 0.5, 0.5), (1, 0, 0), status=0), _hit((0.5, 0.5, 0.5), (1, 0, 0), fresh=0)):
        try:
            host.pick_grid_voxel(bad, (floats, ints), 1)
            raise AssertionError("expected a ValueError")
        except ValueError:
            pass


def test_region_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = [r for r in kernel_resources.collect("tdt_region.hip") if "region_" in r["name"]]
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"region_brush_kernel", "region_merge_v_kernel", "region_merge_b_kernel"} <= names
    # the keys, last-of-run unique and gather kernels are the list layer's (resources: test_bitvol_api.py)
    shared = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in kernel_resources.collect("tdt_voxlist.hip")}
    assert {"voxlist_keys_kernel", "voxlist_last_flags_kernel", "voxlist_unique_kernel", "voxlist_gather_kernel"} <= shared
    assert not {"region_vkeys_kernel", "region_last_flags_kernel", "region_unique_kernel", "region_gather_kernel"} & names
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]
