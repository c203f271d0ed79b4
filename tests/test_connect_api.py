"""Connected components without a GPU: the entry points are exported and bound, the Python tdt_component / tdt_select layouts
are the header's, the kernels of tdt_connect.hip cross-compile without scratch or spills, and the numpy model the GPU tests
compare against equals a plain breadth-first flood fill."""
import collections
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import connect_model as cm
from test_gpu_region_edit import morton
from tdt4230_project_raytracing_amd import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_octree_components", "tdt_octree_edit_connected", "tdt_octree_extract_connected")


def test_connect_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n


def _fields(text, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in re.findall(r"\b(u?int32_t)\s+([^;]+);", body):
        for f in decl[1].split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", f)
            out.append((decl[0], m.group(1), int(m.group(2)) if m.group(2) else 1))
    return out


def test_component_and_select_structs_match_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    comp = _fields(text, "tdt_component")
    assert [f[1] for f in comp] == list(rt.COMPONENT_DTYPE.names)
    offset = 0
    for kind, name, count in comp:
        dt, off = rt.COMPONENT_DTYPE.fields[name][:2]
        assert off == offset, name
        assert dt.base == np.dtype("<u4" if kind == "uint32_t" else "<i4"), name
        assert dt.itemsize == 4 * count, name
        offset += 4 * count
    assert offset == rt.COMPONENT_DTYPE.itemsize == 40
    assert re.search(r"sizeof\(tdt_component\) == 40", text)
    sel = _fields(text, "tdt_select")
    assert [f[1] for f in sel] == [f[0] for f in rt.Select._fields_]
    offset = 0
    for kind, name, count in sel:
        assert count == 1 and getattr(rt.Select, name).offset == offset, name
        want = ctypes.c_uint32 if kind == "uint32_t" else ctypes.c_int32
        assert dict(rt.Select._fields_)[name] is want, name
        offset += 4
    assert offset == ctypes.sizeof(rt.Select) == 24
    assert re.search(r"sizeof\(tdt_select\) == 24", text)
    for name, value in (("TDT_MATCH_ANY", rt.MATCH_ANY), ("TDT_MATCH_MATERIAL", rt.MATCH_MATERIAL)):
        assert re.search(rf"\b{name} = {value}\b", text), name
    assert (cm.MATCH_ANY, cm.MATCH_MATERIAL) == (rt.MATCH_ANY, rt.MATCH_MATERIAL)


def test_connect_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_connect.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"connect_hook_kernel", "connect_flatten_kernel", "connect_table_kernel", "connect_seed_kernel", "connect_touch_kernel",
            "connect_select_kernel"} <= names
    assert sum("connect_hook_kernel<" in r["name"] for r in rows) == 2          # 6 and 26
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


# ---- the model against a breadth-first flood fill ---------------------------------------------------------------------
def flood_fill(grid, connectivity, match):
    """Component of every occupied cell of a dense grid of m = material + 1 (0: empty), numbered by a breadth-first fill that
    starts from each unvisited voxel in Morton order; -1 on empty cells."""
    n = grid.shape[0]
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    occ = np.argwhere(grid > 0)
    occ = occ[np.argsort(morton(occ), kind="stable")]
    comp = -np.ones(grid.shape, np.int64)
    c = 0
    for start in map(tuple, occ):
        if comp[start] >= 0:
            continue
        comp[start] = c
        q = collections.deque([start])
        while q:
            p = q.popleft()
            for d in offs:
                r = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if min(r) < 0 or max(r) >= n or grid[r] == 0 or comp[r] >= 0:
                    continue
                if match == cm.MATCH_MATERIAL and grid[r] != grid[p]:
                    continue
                comp[r] = c
                q.append(r)
        c += 1
    return comp


@pytest.mark.parametrize("side", [5, 9, 12])
def test_model_equals_a_breadth_first_flood_fill(side):
    rng = np.random.default_rng(side)
    depth = int(np.ceil(np.log2(side)))
    checked = 0
    for density in (0.1, 0.3, 0.5, 0.8):
        grid = np.zeros((side,) * 3, np.int64)
        full = rng.random(grid.shape) < density
        grid[full] = rng.integers(1, 4, int(full.sum()))          # three materials, so MATERIAL splits pieces ANY joins
        xyz = np.argwhere(grid > 0)
        V = np.concatenate([xyz, grid[tuple(xyz.T)][:, None]], 1)
        V = V[np.argsort(morton(V[:, :3]), kind="stable")].astype(np.int32)
        for connectivity in (6, 26):
            for match in (cm.MATCH_ANY, cm.MATCH_MATERIAL):
                want = flood_fill(grid, connectivity, match)[tuple(V[:, :3].T)]
                labels, tab = cm.components(V, depth, connectivity, match)
                assert np.array_equal(labels, want), (density, connectivity, match)
                assert len(tab) == want.max() + 1 if len(V) else len(tab) == 0
                assert np.array_equal(tab["voxels"], np.bincount(want, minlength=len(tab)))
                assert np.array_equal(labels[tab["first"]], np.arange(len(tab)))
                assert (np.diff(tab["first"].astype(np.int64)) > 0).all()
                assert np.array_equal(tab["material"], V[tab["first"], 3])
                for c in range(len(tab)):
                    p = V[labels == c, :3]
                    assert list(tab["lo"][c]) == list(p.min(0)) and list(tab["hi"][c]) == list(p.max(0))
                checked += 1
    assert checked == 16


def test_model_selection_and_edits_on_a_small_scene():
    # three pieces: a 2x2x2 block of material 3, a single voxel of material 3 touching it at a corner, a bar of material 5
    # touching the block along a face
    V = [(0, 0, 0, 3), (0, 0, 1, 3), (0, 1, 0, 3), (0, 1, 1, 3), (1, 0, 0, 3), (1, 0, 1, 3), (1, 1, 0, 3), (1, 1, 1, 3),
         (2, 2, 2, 3), (2, 0, 0, 5), (3, 0, 0, 5)]
    V = np.array(V, np.int32)
    V = V[np.argsort(morton(V[:, :3]), kind="stable")]
    depth = 2
    labels, tab = cm.components(V, depth, 6, cm.MATCH_ANY)
    assert list(tab["voxels"]) == [10, 1]
    labels, tab = cm.components(V, depth, 26, cm.MATCH_ANY)
    assert list(tab["voxels"]) == [11]
    labels, tab = cm.components(V, depth, 6, cm.MATCH_MATERIAL)
    assert sorted(tab["voxels"]) == [1, 2, 8]
    # debris: pieces of fewer than 3 voxels at 6 / MATERIAL are the bar and the single voxel
    left = cm.edit(V, depth, rt.REGION_CLEAR, connectivity=6, match=cm.MATCH_MATERIAL, min_voxels=1, max_voxels=2)
    assert len(left) == 8 and (left[:, 3] == 3).all()
    # paint bucket on the bar
    painted = cm.edit(V, depth, rt.REGION_PAINT, material=8, match=cm.MATCH_MATERIAL, seeds=[(3, 0, 0)])
    assert sorted(painted[:, 3]) == [3] * 9 + [9, 9]
    # floating: anchored on the plane x = 0, 6 / ANY keeps the block and bar, drops the corner voxel; a seed on air does nothing
    anchored = cm.edit(V, depth, rt.REGION_CLEAR, regions=[rt.box((0, 0, 0), (0, 3, 3))], invert=True)
    assert len(anchored) == 10
    assert len(cm.edit(V, depth, rt.REGION_CLEAR, seeds=[(3, 3, 3), (-1, 0, 0)])) == len(V)
    assert len(cm.extract(V, depth, seeds=[(2, 2, 2)])) == 1


def test_python_selection_arguments():
    # the size window is checked before ctypes could wrap it
    for lo, hi in ((-1, 5), (0, 2**32), (-(2**31), 0)):
        with pytest.raises(ValueError):
            rt.Context._select(6, rt.MATCH_ANY, lo, hi, False)
    s = rt.Context._select(26, rt.MATCH_MATERIAL, 3, 2**32 - 1, True)
    assert (s.connectivity, s.match, s.min_voxels, s.max_voxels, s.invert) == (26, 1, 3, 2**32 - 1, 1)
    # None: no filter; an empty list: a filter that matches nothing (an off-grid seed, an empty box)
    assert rt._seeds(None) == (None, 0) and rt._touch_regions(None) == (None, 0)
    arr, n = rt._seeds([])
    assert n == 1 and arr.dtype == np.int32 and (arr < 0).all()
    arr, n = rt._seeds([(1, 2, 3), (4, 5, 6)])
    assert n == 2 and arr.tolist() == [[1, 2, 3], [4, 5, 6]]
    arr, k = rt._touch_regions([])
    assert k == 1 and arr[0].shape == rt.SHAPE_BOX and all(arr[0].a[i] > arr[0].b[i] for i in range(3))
    arr, k = rt._touch_regions(rt.sphere((1, 2, 3), 4))
    assert k == 1 and arr[0].shape == rt.SHAPE_SPHERE
