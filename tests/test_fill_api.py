"""Enclosed space without a GPU: the entry points are exported and bound, the Python tdt_fill layout is the header's, the kernels
of tdt_fill.hip cross-compile without scratch or spills, the wrapper checks its arguments, and the numpy model the GPU tests
compare against (tests/fill_model.py) equals an independent breadth-first search, the closed forms of the definition, and the
plane test of convex meshes."""
import ctypes
import os
import re
import sys
from collections import deque

import numpy as np
import pytest

import fill_model as fm
import mesh_model as mm
from morph_model import offsets
from test_gpu_connect import block
from tdt4230_project_raytracing_amd import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_octree_extract_enclosed", "tdt_octree_fill_enclosed", "tdt_voxelize_triangles_solid", "tdt_octree_edit_triangles_solid")
U = mm.UNIT


def test_fill_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES + ("tdt_debug_fill_passes",):
        assert hasattr(L, n), n
        assert n in bound, n
    for n in ("octree_extract_enclosed", "octree_fill_enclosed", "voxelize_triangles_solid", "octree_edit_triangles_solid"):
        assert callable(getattr(rt.Context, n)), n


def test_fill_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_fill \{(.*?)\} tdt_fill;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"int32_t\s+(\w+);", body)
    assert fields == [f[0] for f in rt.Fill._fields_] == ["connectivity", "material"]
    for i, name in enumerate(fields):
        assert getattr(rt.Fill, name).offset == 4 * i and dict(rt.Fill._fields_)[name] is ctypes.c_int32
    assert ctypes.sizeof(rt.Fill) == 8
    assert len(re.findall(r"sizeof\(tdt_fill\) == 8", text)) == 2            # C++ and C


def test_fill_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_fill.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"fill_seed_kernel", "fill_flood_kernel", "fill_count_kernel", "fill_emit_kernel"} <= names     # the shared steps: test_bitvol_api.py
    assert sum("fill_flood_kernel<" in r["name"] for r in rows) == 2         # connectivity 6 and 26
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


def test_python_wrapper_argument_checks():
    f = rt.Context._fill(26, None)
    assert (f.connectivity, f.material) == (26, -1)
    f = rt.Context._fill(6, 253)
    assert (f.connectivity, f.material) == (6, 253)
    assert rt.Context._fill(7, 999).connectivity == 7                        # the ranges are the library's to check
    for bad in (lambda: rt.Context._fill(True, 0), lambda: rt.Context._fill(6, False), lambda: rt.Context._fill(6.5, 0),
                lambda: rt.Context._fill(6, 2 ** 31), lambda: rt.Context._fill(-2 ** 31 - 1, 0), lambda: rt.Context._fill(6, 1.5)):
        with pytest.raises(ValueError):
            bad()


# ---- the model against a plain breadth-first search ------------------------------------------------------------------------
def bfs_outside(empty, connectivity):
    n = empty.shape[0]
    offs = [d for _, d in offsets(connectivity)]
    seen = np.zeros_like(empty)
    todo = deque()
    for p in np.ndindex(n, n, n):
        if empty[p] and (0 in p or n - 1 in p):
            seen[p] = True
            todo.append(p)
    while todo:
        p = todo.popleft()
        for d in offs:
            q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
            if min(q) >= 0 and max(q) < n and empty[q] and not seen[q]:
                seen[q] = True
                todo.append(q)
    return seen


@pytest.mark.parametrize("connectivity", [6, 26])
def test_model_equals_a_breadth_first_search(connectivity):
    rng = np.random.default_rng(connectivity)
    pockets = 0
    for n in (4, 5, 6, 7, 8):
        for density in ((0.45, 0.6, 0.75) if connectivity == 6 else (0.7, 0.82, 0.9)):     # pockets under 26 need thick rock
            for _ in range(4):
                empty = rng.random((n, n, n)) >= density
                got = fm.outside(empty, connectivity)
                assert np.array_equal(got, bfs_outside(empty, connectivity)), (n, density)
                assert np.array_equal(fm.outside_sweeps(empty, connectivity), got), (n, density)      # the large-grid form
                pockets += int((empty & ~got).sum())
    assert pockets >= 10


def test_list_form_of_the_model():
    """Morton order, the mask, the fixed material, and inheritance along -x."""
    W = hollow((1, 1, 1), (6, 5, 5))                                          # inner 4 x 3 x 3
    W[:, 3] = 1 + W[:, 1]                                                     # the wall's material depends on y
    W = np.concatenate([W, [[3, 3, 3, 77]]]).astype(np.int32)                 # and a pillar voxel inside
    E = fm.enclosed(W, 3)
    assert len(E) == 4 * 3 * 3 - 1
    k = fm.keys(E[:, :3])
    assert (k[1:] > k[:-1]).all()
    for x, y, z, m in E:
        assert m == (77 if (y, z) == (3, 3) and x > 3 else 1 + y)
    assert set(fm.enclosed(W, 3, material=9)[:, 3]) == {10}
    half = fm.enclosed(W, 3, regions=rt.box((0, 0, 0), (3, 7, 7)))
    assert np.array_equal(half, E[E[:, 0] <= 3]) and 0 < len(half) < len(E)
    assert len(fm.enclosed(W, 3, regions=[])) == 0
    both = fm.filled(W, 3)
    assert len(both) == len(W) + len(E) and np.array_equal(both[np.isin(fm.keys(both[:, :3]), fm.keys(W[:, :3]))], fm._sorted(W))


# ---- closed forms ------------------------------------------------------------------------------------------------------------
def hollow(lo, hi, m=1):
    """A box lo..hi with walls one voxel thick."""
    b = block(lo, hi, m)
    inner = (b[:, :3] > np.array(lo)).all(1) & (b[:, :3] < np.array(hi)).all(1)
    return b[~inner]


def without(W, *voxels):
    keep = np.ones(len(W), bool)
    for v in voxels:
        hit = (W[:, :3] == np.array(v)).all(1)
        assert hit.sum() == 1, v
        keep &= ~hit
    return W[keep]


@pytest.mark.parametrize("inner", [(1, 1, 1), (2, 1, 3), (4, 5, 2), (6, 6, 6)])
def test_hollow_box_closed_forms(inner):
    a, b, c = inner
    lo, hi = (1, 1, 1), (2 + a, 2 + b, 2 + c)
    W = hollow(lo, hi)
    for conn in (6, 26):
        E = fm.enclosed(W, 4, conn)
        assert len(E) == a * b * c
        assert E[:, :3].min(0).tolist() == [2, 2, 2] and E[:, :3].max(0).tolist() == [1 + a, 1 + b, 1 + c]
        # a wall voxel removed in the middle of a face: everything drains
        hole = (lo[0], 2 + (b - 1) // 2, 2 + (c - 1) // 2)
        assert len(fm.enclosed(without(W, hole), 4, conn)) == 0
    # an edge voxel of the wall removed: the inside touches the outside along an edge only; a corner voxel: by a corner only
    for gap in ((lo[0], lo[1], 2), (lo[0], lo[1], lo[2])):
        assert len(fm.enclosed(without(W, gap), 4, 6)) == a * b * c
        assert len(fm.enclosed(without(W, gap), 4, 26)) == 0


def test_a_box_open_to_a_grid_face_is_not_enclosed():
    n = 8
    W = hollow((0, 2, 2), (4, 6, 6))
    assert len(fm.enclosed(W, 3)) == 3 * 3 * 3                                # its wall lies ON the face x = 0: still closed
    open_box = W[W[:, 0] > 0]                                                 # that wall removed: the cavity reaches the face
    for conn in (6, 26):
        assert len(fm.enclosed(open_box, 3, conn)) == 0
    full = block((0, 0, 0), (n - 1, n - 1, n - 1))
    assert len(fm.enclosed(full, 3)) == 0 and len(fm.enclosed(full[:0], 3)) == 0
    assert len(fm.enclosed(without(full, (3, 4, 5)), 3, 26)) == 1


# ---- convex meshes: the fill is the plane test -------------------------------------------------------------------------------
def convex_cases():
    cube_v = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.int64)
    cube_t = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7),
                       (1, 7, 3)], np.uint32)
    octa_v = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64)
    octa_t = np.array([(a, b, c) for a in (0, 1) for b in (2, 3) for c in (4, 5)], np.uint32)
    sv, st = mm.uv_sphere((8.3, 7.6, 8.1), 6.2, 6, 8)
    return {
        "cube": (cube_v * (19 * U + 7) + (5 * U + 3, 4 * U + 9, 6 * U + 1), cube_t, 5),
        "octahedron": (octa_v * (12 * U + 5) + (16 * U, 15 * U + 31, 17 * U + 2), octa_t, 5),
        "uv_sphere": (mm.quantize(sv), st, 4),
    }


@pytest.mark.parametrize("name", list(convex_cases()))
def test_convex_mesh_fill_is_the_plane_test(name):
    v, t, depth = convex_cases()[name]
    n = 1 << depth
    assert v.min() > 0 and v.max() < n * U                                   # strictly inside the grid
    S = mm.voxelize(v.astype(np.int32), t, depth)
    # centres strictly inside every face plane, in Python integers; each face is oriented by the vertex sum
    P = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    c = (P * U + U // 2).astype(object)
    vo = v.astype(object)
    total, count = vo.sum(0), len(vo)
    strictly = np.ones(len(P), bool)
    for tri in t:
        a, b, d = vo[tri[0]], vo[tri[1]], vo[tri[2]]
        e0, e1 = b - a, d - a
        nrm = np.array([e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]], object)
        side = int((nrm * (total - count * a)).sum())
        assert side != 0
        s = ((c - a) * nrm).sum(1)
        strictly &= np.array([(int(x) > 0) == (side > 0) and int(x) != 0 for x in s])
    covered = np.zeros(len(P), bool)
    covered[(S[:, 0].astype(np.int64) * n + S[:, 1]) * n + S[:, 2]] = True
    want = P[strictly & ~covered]
    assert len(want) > 0
    for conn in (6, 26):
        solid = fm.filled(S, depth, conn)
        extra = solid[~np.isin(fm.keys(solid[:, :3]), fm.keys(S[:, :3]))]
        assert {tuple(p) for p in extra[:, :3]} == {tuple(p) for p in want}, (name, conn)
