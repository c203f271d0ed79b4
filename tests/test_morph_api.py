"""Voxel morphology without a GPU: the entry points are exported and bound, the Python tdt_morph layout is the header's, the
kernels of tdt_morph.hip cross-compile without scratch or spills, the numpy model the GPU tests compare against equals an
independent dense-grid restatement and the closed forms of the semantics, and the wrapper checks its arguments."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

import morph_model as mm
from test_connect_api import _fields
from test_gpu_region_edit import morton, sort_vox
from tdt4230_project_raytracing_amd import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_octree_morph", "tdt_octree_extract_morph")
OPS = (mm.DILATE, mm.ERODE, mm.OPEN, mm.CLOSE, mm.SHELL)


def test_morph_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n


def test_morph_struct_and_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    fields = _fields(text, "tdt_morph")
    assert [f[1] for f in fields] == [f[0] for f in rt.Morph._fields_] == ["op", "connectivity", "radius", "material", "border", "pad"]
    offset = 0
    for kind, name, count in fields:
        assert kind == "int32_t" and count == 1 and getattr(rt.Morph, name).offset == offset, name
        assert dict(rt.Morph._fields_)[name] is ctypes.c_int32, name
        offset += 4
    assert offset == ctypes.sizeof(rt.Morph) == 24
    assert len(re.findall(r"sizeof\(tdt_morph\) == 24", text)) == 2          # C++ and C
    for name, value in (("TDT_MORPH_DILATE", rt.MORPH_DILATE), ("TDT_MORPH_ERODE", rt.MORPH_ERODE), ("TDT_MORPH_OPEN", rt.MORPH_OPEN),
                        ("TDT_MORPH_CLOSE", rt.MORPH_CLOSE), ("TDT_MORPH_SHELL", rt.MORPH_SHELL)):
        assert re.search(rf"\b{name} = {value}\b", text), name
    assert (rt.MORPH_DILATE, rt.MORPH_ERODE, rt.MORPH_OPEN, rt.MORPH_CLOSE, rt.MORPH_SHELL) == (0, 1, 2, 3, 4)


def test_morph_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_morph.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"morph_probe_kernel", "morph_emit_kernel", "morph_unique_kernel", "morph_merge_list_kernel", "morph_merge_new_kernel",
            "morph_select_kernel", "morph_mask_result_kernel", "morph_mask_tree_kernel"} <= names
    # the keys and gather kernels are the list layer's (resources: test_bitvol_api.py)
    shared = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in kernel_resources.collect("tdt_voxlist.hip")}
    assert {"voxlist_keys_kernel", "voxlist_gather_kernel"} <= shared and not {"morph_keys_kernel", "morph_gather_kernel"} & names
    assert sum("morph_probe_kernel<6>" in r["name"] for r in rows) == 1
    assert sum("morph_probe_kernel<26>" in r["name"] for r in rows) == 1
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


def test_gallop_find_has_one_definition():
    csrc = os.path.join(ROOT, "tdt4230_project_raytracing_amd", "csrc")
    owners = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".h"))
              and re.search(r"int gallop_find\(", open(os.path.join(csrc, f)).read())]
    assert owners == ["region_device.hpp"]


# ---- the model against a dense-grid restatement ------------------------------------------------------------------------
def shifted(a, d, fill):
    """s[p] = a[p + d], `fill` where p + d is outside the array."""
    n = a.shape[0]
    p = np.pad(a, 1, constant_values=fill)
    return p[1 + d[0]: 1 + d[0] + n, 1 + d[1]: 1 + d[1] + n, 1 + d[2]: 1 + d[2] + n]


def dense_offsets(connectivity):
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    return [d for d in offs if connectivity == 26 or sum(map(abs, d)) == 1]   # itertools order = ascending t


def dense_dilate(g, connectivity, material):
    out = g.copy()
    new = np.zeros_like(g)
    for d in reversed(dense_offsets(connectivity)):      # descending t: the last write, the lowest t, wins
        s = shifted(g, d, 0)
        new[s > 0] = s[s > 0]
    fresh = (g == 0) & (new > 0)
    out[fresh] = material + 1 if material is not None else new[fresh]
    return out


def dense_erode(g, connectivity, border):
    keep = g > 0
    for d in dense_offsets(connectivity):
        keep &= shifted(g > 0, d, bool(border))
    return np.where(keep, g, 0)


def dense_morph(g, op, radius, connectivity, material, border, mask):
    def rep(f, a, *args):
        for _ in range(radius):
            a = f(a, *args)
        return a
    if op == mm.DILATE:
        r = rep(dense_dilate, g, connectivity, material)
    elif op == mm.ERODE:
        r = rep(dense_erode, g, connectivity, border)
    elif op == mm.OPEN:
        r = np.where(rep(dense_dilate, rep(dense_erode, g, connectivity, 1), connectivity, material) > 0, g, 0)   # original materials
    elif op == mm.CLOSE:
        r = rep(dense_erode, rep(dense_dilate, g, connectivity, material), connectivity, 1)
    else:
        r = np.where(rep(dense_erode, g, connectivity, border) > 0, 0, g)
    return r if mask is None else np.where(mask, r, g)


def to_list(g):
    xyz = np.argwhere(g > 0)
    return sort_vox(np.concatenate([xyz, g[tuple(xyz.T)][:, None]], 1))


@pytest.mark.parametrize("side", [5, 9, 12])
def test_model_equals_the_dense_grid_restatement(side):
    rng = np.random.default_rng(100 + side)
    depth = int(np.ceil(np.log2(side)))
    N = 1 << depth
    regions = [rt.box((1, 0, 2), (side - 2, side // 2, N)), rt.sphere((side // 2, side // 2, side // 2), side // 3)]
    gx, gy, gz = np.meshgrid(*[np.arange(N)] * 3, indexing="ij")
    c, r = side // 2, side // 3
    dense_mask = (((gx >= 1) & (gx <= side - 2) & (gy >= 0) & (gy <= side // 2) & (gz >= 2) & (gz <= N))
                  | ((gx - c) ** 2 + (gy - c) ** 2 + (gz - c) ** 2 <= r * r))
    checked = 0
    for density in (0.1, 0.3, 0.5, 0.8):
        g = np.zeros((N,) * 3, np.int64)
        full = rng.random((side,) * 3) < density
        g[:side, :side, :side][full] = rng.integers(1, 4, int(full.sum()))     # three materials
        V = to_list(g)
        for op, conn, radius, border, material, masked in itertools.product(OPS, (6, 26), (1, 2, 3), (0, 1), (None, 6), (False, True)):
            got = mm.morph(V, depth, op, radius, conn, material, border, regions if masked else None)
            want = to_list(dense_morph(g, op, radius, conn, material, border, dense_mask if masked else None))
            assert np.array_equal(got, want), (density, op, conn, radius, border, material, masked)
            checked += 1
    assert checked == 4 * 5 * 2 * 3 * 2 * 2 * 2


def test_model_keys_are_the_morton_keys():
    xyz = np.random.default_rng(3).integers(0, 1024, (5000, 3))
    assert np.array_equal(mm._keys(xyz), morton(xyz).astype(np.int64))
    v = np.concatenate([xyz[:50], np.ones((50, 1), np.int64)], 1)
    assert np.array_equal(mm._sorted(v), sort_vox(v))
    k = mm._keys(xyz)
    inner = ((xyz > 0) & (xyz < 1023)).all(1)
    for _, d in mm.offsets(26):
        assert np.array_equal(mm._shift_keys(k[inner], d), mm._keys(xyz[inner] + np.array(d)))


# ---- closed forms ------------------------------------------------------------------------------------------------------
def block(lo, hi, m=1):
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([g, np.full((len(g), 1), m)], 1).astype(np.int32)


def test_dilate_of_one_voxel_is_the_ball_of_the_structuring_element():
    depth = 6
    mid = np.array([[32, 32, 32, 5]], np.int32)
    for r, want6 in ((1, 7), (2, 25), (3, 63)):
        assert want6 == (2 * r + 1) * (2 * r * r + 2 * r + 3) // 3
        d6 = mm.morph(mid, depth, mm.DILATE, r, 6)
        assert len(d6) == want6 and (np.abs(d6[:, :3] - 32).sum(1) <= r).all() and (d6[:, 3] == 5).all()
        d26 = mm.morph(mid, depth, mm.DILATE, r, 26)
        assert len(d26) == (2 * r + 1) ** 3 and (np.abs(d26[:, :3] - 32).max(1) <= r).all()
        # at the grid's corner: the clipped octant
        corner = np.array([[0, 0, 0, 2]], np.int32)
        c6 = mm.morph(corner, depth, mm.DILATE, r, 6)
        assert len(c6) == (r + 1) * (r + 2) * (r + 3) // 6 and (c6[:, :3] >= 0).all() and (c6[:, :3].sum(1) <= r).all()
        c26 = mm.morph(corner, depth, mm.DILATE, r, 26, material=8)
        assert len(c26) == (r + 1) ** 3 and (c26[:, :3] >= 0).all()
        assert sorted(c26[:, 3]) == [2] + [9] * ((r + 1) ** 3 - 1)


def test_erode_and_shell_of_a_solid_block():
    depth, n = 5, 12
    V = sort_vox(block((4, 5, 6), (4 + n - 1, 5 + n - 1, 6 + n - 1), 3))
    for conn in (6, 26):
        for r in (1, 2, 3):
            E = mm.morph(V, depth, mm.ERODE, r, conn)
            assert len(E) == (n - 2 * r) ** 3
            assert (E[:, :3].min(0) == np.array([4, 5, 6]) + r).all() and (E[:, :3].max(0) == np.array([4, 5, 6]) + n - 1 - r).all()
            S = mm.morph(V, depth, mm.SHELL, r, conn)
            both = sort_vox(np.concatenate([S, E]))
            assert np.array_equal(both, V) and len(S) + len(E) == len(V)
            assert not np.isin(morton(S[:, :3]), morton(E[:, :3])).any()
    # a grid-filling solid: border 1 never erodes, border 0 peels the outer layer
    full = sort_vox(block((0, 0, 0), (7, 7, 7), 2))
    assert len(mm.morph(full, 3, mm.SHELL, 1, 26, border=1)) == 0
    assert np.array_equal(mm.morph(full, 3, mm.ERODE, 2, 6, border=1), full)
    assert len(mm.morph(full, 3, mm.SHELL, 1, 6, border=0)) == 8 ** 3 - 6 ** 3
    assert len(mm.morph(full, 3, mm.ERODE, 4, 6, border=0)) == 0


def test_open_and_close_are_an_adjunction():
    rng = np.random.default_rng(7)
    depth, N = 4, 16
    for density in (0.2, 0.5, 0.8):
        g = np.where(rng.random((N,) * 3) < density, rng.integers(1, 4, (N,) * 3), 0)      # up to the grid faces
        V = to_list(g)
        kv = morton(V[:, :3])
        for conn in (6, 26):
            for r in (1, 2):
                O = mm.morph(V, depth, mm.OPEN, r, conn, border=0)
                C = mm.morph(V, depth, mm.CLOSE, r, conn, border=0)
                ko, kc = morton(O[:, :3]), morton(C[:, :3])
                assert np.isin(ko, kv).all() and np.isin(kv, kc).all()
                assert np.array_equal(O, V[np.isin(kv, ko)])                   # OPEN keeps the original materials
                assert np.array_equal(C[np.isin(kc, kv)], V)                   # CLOSE leaves V's materials alone
                assert np.array_equal(mm.morph(O, depth, mm.OPEN, r, conn), O)
                assert np.array_equal(mm.morph(C, depth, mm.CLOSE, r, conn), C)
                assert np.array_equal(mm.morph(V, depth, mm.OPEN, r, conn, border=1), O)    # border is ignored


def test_inherit_takes_the_first_offset_in_ascending_t():
    # an empty voxel between material 3 at -x and material 8 at +x: d = (-1, 0, 0) has t = 4, d = (1, 0, 0) t = 22
    V = np.array([[3, 4, 4, 4], [5, 4, 4, 9]], np.int32)
    D = mm.morph(V, 3, mm.DILATE, 1, 6)
    assert D[(D[:, :3] == (4, 4, 4)).all(1), 3].tolist() == [4]
    # at 26 the voxel (4, 5, 4) sees (3, 4, 4) through d = (-1, -1, 0), t = 1, before (5, 4, 4) through (1, -1, 0), t = 19
    D = mm.morph(V, 3, mm.DILATE, 1, 26)
    assert D[(D[:, :3] == (4, 5, 4)).all(1), 3].tolist() == [4]
    # (6, 4, 4) has only the material-8 voxel in reach
    assert D[(D[:, :3] == (6, 4, 4)).all(1), 3].tolist() == [9]


def test_python_morph_arguments():
    m = rt.Context._morph(rt.MORPH_CLOSE, 3, 26, None, 1)
    assert (m.op, m.connectivity, m.radius, m.material, m.border, m.pad) == (3, 26, 3, -1, 1, 0)
    assert rt.Context._morph(rt.MORPH_DILATE, 1, 6, 253, 0).material == 253
    # values ctypes would wrap into a valid int32, and values that are not integers, never reach the library
    for bad in (dict(radius=2**32 + 1), dict(radius=1.5), dict(connectivity=2**32 + 6), dict(material=2**32 + 3), dict(material=-2**31 - 1),
                dict(op=2**32), dict(border=2**32), dict(op="dilate"), dict(radius=True)):
        kw = dict(op=rt.MORPH_DILATE, radius=1, connectivity=6, material=None, border=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            rt.Context._morph(**kw)
    assert rt._touch_regions(None) == (None, 0)
