"""Stroke brushes without a GPU: the entry points are exported and bound, the Python tdt_stroke layout is the header's, the unit
is part of the device library and its kernels cross-compile without scratch or spills, the wrapper refuses every bad argument the
header lists, and the numpy model the GPU tests compare against (tests/stroke_model.py) equals a brute force in exact rationals
and the closed forms of the definition."""
import ctypes
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import stroke_model as sm
from test_gpu_region_edit import brush_voxels
from tdt4230_project_raytracing_amd import build, rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_voxelize_stroke", "tdt_octree_edit_stroke", "tdt_octree_extract_stroke")
NIBS = (rt.SHAPE_SPHERE, rt.SHAPE_BOX)


@pytest.fixture(autouse=True)
def model_states_the_library_contract():
    """The model is a restatement of the library's contract: its shapes and limits are the wrapper's, or nothing below means anything."""
    assert (sm.SPHERE, sm.BOX) == (rt.SHAPE_SPHERE, rt.SHAPE_BOX)
    assert (sm.COORD_MAX, sm.RADIUS_MAX) == (rt.STROKE_COORD_MAX, rt.STROKE_RADIUS_MAX)


def test_stroke_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    assert "tdt_stroke.hip" in build.DEVICE_UNITS
    assert os.path.exists(os.path.join(build.CSRC, "tdt_stroke.hip"))


def test_stroke_struct_and_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_stroke \{(.*?)\} tdt_stroke;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for kind, names in re.findall(r"((?:const\s+)?u?int32_t\s*\*?)\s*([^;]+);", body):
        pointer = "*" in kind or names.strip().startswith("*")
        base = "uint32_t" if "uint32_t" in kind else "int32_t"
        for f in names.split(","):
            fields.append((base, pointer, f.strip().lstrip("*")))
    assert [f[2] for f in fields] == [f[0] for f in rt.Stroke._fields_] == ["points", "segments", "materials", "n_points", "n_segments", "shape",
                                                                          "radius", "material", "pad"]
    offset = 0
    for base, pointer, name in fields:
        ctype = dict(rt.Stroke._fields_)[name]
        assert getattr(rt.Stroke, name).offset == offset, name
        assert ctype is (ctypes.c_void_p if pointer else ctypes.c_uint32 if base == "uint32_t" else ctypes.c_int32), name
        offset += 8 if pointer else 4
    assert offset == ctypes.sizeof(rt.Stroke) == 48
    assert len(re.findall(r"sizeof\(tdt_stroke\) == 48", text)) == 2          # C++ and C
    assert re.search(r"#define TDT_STROKE_COORD_MAX 8192\b", text) and rt.STROKE_COORD_MAX == sm.COORD_MAX == 8192
    assert re.search(r"#define TDT_STROKE_RADIUS_MAX 2048\b", text) and rt.STROKE_RADIUS_MAX == sm.RADIUS_MAX == 2048
    assert (sm.SPHERE, sm.BOX) == (rt.SHAPE_SPHERE, rt.SHAPE_BOX)


def test_stroke_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_stroke.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"stroke_setup_kernel", "stroke_tiles_kernel", "stroke_pairs_kernel", "stroke_voxels_kernel", "stroke_emit_kernel"} <= names
    assert sum("stroke_voxels_kernel<" in r["name"] for r in rows) == 4       # count / emit x round / cube nib
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


# ---- the wrapper's argument checks -------------------------------------------------------------------------------------------
def test_python_wrapper_argument_checks():
    p = np.array([[0, 0, 0], [5, 6, 7], [9, 9, 9]], np.int32)
    s, keep = rt._stroke(p, 3, None, [5, 9], 7, rt.SHAPE_BOX)
    assert (s.n_points, s.n_segments, s.shape, s.radius, s.material, s.pad) == (3, 0, rt.SHAPE_BOX, 3, 7, 0)
    assert s.points == keep[0].ctypes.data and s.segments is None and s.materials == keep[2].ctypes.data and keep[2].dtype == np.int32
    s, keep = rt._stroke(p, 0, [[0, 2], [1, 1]], [1, 254])
    assert (s.n_segments, s.shape) == (2, rt.SHAPE_SPHERE) and s.segments == keep[1].ctypes.data and keep[1].dtype == np.uint32
    empty, _ = rt._stroke(np.zeros((0, 3), np.int32), 2)
    assert (empty.points, empty.segments, empty.materials, empty.n_points, empty.n_segments) == (None, None, None, 0, 0)
    none, _ = rt._stroke(p, 2, np.zeros((0, 2), np.uint32))                  # an explicit empty list is not the polyline
    assert none.segments is not None and none.n_segments == 0
    one, _ = rt._stroke(p[:1], 2, None, [4])                                 # one point: one dab, one material
    assert (one.n_points, one.n_segments) == (1, 0)
    edge = p.copy()
    edge[0] = [rt.STROKE_COORD_MAX, -rt.STROKE_COORD_MAX, 0]
    rt._stroke(edge, rt.STROKE_RADIUS_MAX, None, None, 253, depth=10, op=rt.REGION_CLEAR)
    far, neg = p.copy(), p.copy()
    far[1, 2] = rt.STROKE_COORD_MAX + 1
    neg[2, 0] = -rt.STROKE_COORD_MAX - 1
    for bad in (lambda: rt._stroke(p.astype(np.float32), 1),                  # float points
                lambda: rt._stroke(p[:, :2], 1),
                lambda: rt._stroke(p.astype(np.int64) + 2 ** 40, 1),
                lambda: rt._stroke(far, 1), lambda: rt._stroke(neg, 1),       # a coordinate out of range
                lambda: rt._stroke(p, 1, [[0, 3]]),                           # an index >= n_points
                lambda: rt._stroke(p, 1, [[0, -1]]),                          # an index that would wrap
                lambda: rt._stroke(p, 1, [[0, 2 ** 32]]),
                lambda: rt._stroke(p, 1, [[0, 1, 2]]),
                lambda: rt._stroke(np.zeros((0, 3), np.int32), 1, [[0, 0]]),  # n_points = 0 with segments
                lambda: rt._stroke(p, -1), lambda: rt._stroke(p, rt.STROKE_RADIUS_MAX + 1), lambda: rt._stroke(p, 1.5),
                lambda: rt._stroke(p, True),
                lambda: rt._stroke(p, 1, None, [1]),                          # one material per segment
                lambda: rt._stroke(p, 1, [[0, 1]], [1, 2]),
                lambda: rt._stroke(p, 1, None, [0, 1]), lambda: rt._stroke(p, 1, None, [1, 255]), lambda: rt._stroke(p, 1, None, [1.5, 2]),
                lambda: rt._stroke(p, 1, None, None, -1), lambda: rt._stroke(p, 1, None, None, 254), lambda: rt._stroke(p, 1, None, None, 2 ** 31),
                lambda: rt._stroke(p, 1, shape=2), lambda: rt._stroke(p, 1, shape=-1),
                lambda: rt._stroke(p, 1, depth=0), lambda: rt._stroke(p, 1, depth=11),
                lambda: rt._stroke(p, 1, op=4), lambda: rt._stroke(p, 1, op=-1),
                lambda: rt._stroke(np.zeros(((1 << 20) + 1, 3), np.int32), 1),                         # more than 2^20 points
                lambda: rt._stroke(p, 1, np.zeros(((1 << 20) + 1, 2), np.uint32))):                    # more than 2^20 segments
        with pytest.raises(ValueError):
            bad()


# ---- the model against exact rationals ---------------------------------------------------------------------------------------
def exact_sphere(a, d, r, p):
    """The squared distance from p to the nearest point of the segment, in rationals, against r^2."""
    w = [p[k] - a[k] for k in range(3)]
    L2 = sum(c * c for c in d)
    s = Fraction(0) if L2 == 0 else min(max(Fraction(sum(w[k] * d[k] for k in range(3)), L2), Fraction(0)), Fraction(1))
    return sum((w[k] - s * d[k]) ** 2 for k in range(3)) <= r * r


def exact_box(a, d, r, p):
    """min over s in [0, 1] of max_k |w_k - s d_k|, in rationals, against r.  The function is convex and piecewise linear, so its
    minimum is at an end of [0, 1] or where two of the six lines +-(w_k - s d_k) cross (a line and its own mirror included)."""
    w = [p[k] - a[k] for k in range(3)]
    cand = {Fraction(0), Fraction(1)}
    lines = [(sg * w[k], sg * d[k]) for k in range(3) for sg in (1, -1)]      # value = c - s m
    for i in range(6):
        for j in range(i + 1, 6):
            (c0, m0), (c1, m1) = lines[i], lines[j]
            if m0 != m1:
                s = Fraction(c0 - c1, m0 - m1)
                if 0 < s < 1:
                    cand.add(s)
    return min(max(abs(w[k] - s * d[k]) for k in range(3)) for s in cand) <= r


def test_model_equals_a_brute_force_in_rationals():
    rng = np.random.default_rng(31)
    for n, count in ((8, 30), (16, 5)):
        vox = sm.grid(np.zeros(3, np.int64), np.full(3, n - 1, np.int64))
        for shape, exact in ((rt.SHAPE_SPHERE, exact_sphere), (rt.SHAPE_BOX, exact_box)):
            hits = 0
            for i in range(count):
                a = rng.integers(-n // 2, n + n // 2, 3)
                b = a.copy() if i % 10 == 9 else rng.integers(-n // 2, n + n // 2, 3)
                if i % 10 in (7, 8):                                         # axis-parallel and in-plane segments: zero components of d
                    b[: i % 10 - 6] = a[: i % 10 - 6]
                r = int(rng.integers(0, 4))
                ai, di = [int(c) for c in a], [int(c) for c in b - a]
                want = np.array([exact(ai, di, r, [int(c) for c in p]) for p in vox])
                test = sm.capsule if shape == rt.SHAPE_SPHERE else sm.swept_box
                assert np.array_equal(test(a, b, r, vox), want), (shape, ai, di, r)
                assert np.array_equal(test(b, a, r, vox), want), (shape, ai, di, r)        # (b, a) is the same set
                got = sm.covered(a, b, r, shape, n.bit_length() - 1)
                assert {tuple(p) for p in got} == {tuple(p) for p in vox[want]}            # and the clipped box loses nothing
                hits += int(want.sum())
            assert 0 < hits < count * len(vox)


def test_slabbed_model_equals_the_flat_model():
    """covered() cuts large boxes into slabs along the segment (so that grid-spanning strokes at depth 9 take seconds); on every
    voxel of the clipped box it must find what the plain test finds."""
    rng = np.random.default_rng(17)
    n, cases = 64, 0
    for i in range(60):
        a = rng.integers(-32, n + 32, 3)
        b = a + rng.integers(-3, 4, 3) * (1, 1, 0) if i % 6 == 0 else rng.integers(-32, n + 32, 3)
        if i % 6 == 1:
            b[int(rng.integers(3))] = a[int(rng.integers(3))]
        r = int(rng.choice([0, 1, 2, 5, 11]))
        for shape in NIBS:
            flat = sm.covered_flat(a, b, r, shape, 6)
            got = sm.covered(a, b, r, shape, 6, flat_limit=64)
            assert len(got) == len(flat) and {tuple(p) for p in got} == {tuple(p) for p in flat}, (a, b, r, shape)
            cases += len(flat) > 0
    assert cases > 60


def test_body_diagonal_count():
    # the figure of the contract: a 64^3 body diagonal with the round nib of radius 2
    got = sm.voxelize([[0, 0, 0], [63, 63, 63]], 2, 6)
    assert len(got) == 1186
    # radius 0 on it: the 64 lattice points of the diagonal, both nibs
    for shape in NIBS:
        got = sm.voxelize([[0, 0, 0], [63, 63, 63]], 0, 6, shape=shape)
        assert got[:, :3].tolist() == [[i, i, i] for i in range(64)]


def test_identities():
    rng = np.random.default_rng(7)
    depth, n = 4, 16
    # a dab is the sphere / the box of the region edits
    for c, r in (((5, 6, 7), 3), ((0, 15, 8), 4), ((-2, 3, 17), 5), ((8, 8, 8), 0), ((30, 30, 30), 3)):
        for shape in NIBS:
            region = rt.sphere(c, r) if shape == rt.SHAPE_SPHERE else rt.box(tuple(v - r for v in c), tuple(v + r for v in c))
            want = brush_voxels([region], depth)
            for got in (sm.voxelize([c], r, depth, shape=shape), sm.voxelize([c, c], r, depth, shape=shape),
                        sm.voxelize([c, (1, 1, 1)], r, depth, segments=[[0, 0]], shape=shape)):
                assert {tuple(p) for p in got[:, :3]} == {tuple(p) for p in want}, (c, r, shape)
    # a polyline is the last-wins union of its segments
    pts, mats = sm.random_stroke(rng, 9, n)
    for shape in NIBS:
        whole = sm.voxelize(pts, 2, depth, materials=mats, shape=shape)
        owner = {}
        for s in range(9):
            for x, y, z, m in sm.voxelize(pts[s:s + 2], 2, depth, material=int(mats[s]) - 1, shape=shape):
                owner[(x, y, z)] = m
        assert {tuple(v[:3]): v[3] for v in whole} == owner and len(whole) == len(owner) > 0
        key = sm.morton(whole[:, :3])
        assert (key[1:] > key[:-1]).all()
        # explicit segments in another order: the same set, the materials of the new order
        seg = np.array([[i, i + 1] for i in range(9)])[::-1]
        back = sm.voxelize(pts, 2, depth, segments=seg, materials=mats[::-1], shape=shape)
        assert np.array_equal(back[:, :3], whole[:, :3])
    # radius 0 along an axis: a bar one voxel thick, clipped to the grid
    for shape in NIBS:
        got = sm.voxelize([[-3, 5, 9], [11, 5, 9]], 0, depth, shape=shape, material=8)
        assert got[np.argsort(got[:, 0])].tolist() == [[x, 5, 9, 9] for x in range(12)]
        # and a generic one: only the lattice points on it
        got = sm.voxelize([[1, 2, 3], [7, 5, 15]], 0, depth, shape=shape)
        assert {tuple(p) for p in got[:, :3]} == {(1, 2, 3), (3, 3, 7), (5, 4, 11), (7, 5, 15)}
    # wholly off the grid, the empty stroke, an explicit empty segment list
    assert sm.voxelize([[-9, -9, -9], [-5, 20, -5]], 3, depth).shape == (0, 4)
    assert sm.voxelize(np.zeros((0, 3)), 3, depth).shape == (0, 4)
    assert sm.voxelize(pts, 3, depth, segments=np.zeros((0, 2))).shape == (0, 4)
    # the tile count the first limit is stated in
    assert sm.tile_candidates([0, 0, 0], [1023, 1023, 1023], 2048, 10) == 1 << 21
    assert sm.tile_candidates([8, 8, 8], [15, 15, 15], 0, 5) == 1 and sm.tile_candidates([7, 8, 8], [15, 15, 16], 0, 5) == 4
    assert sm.tile_candidates([-9, 0, 0], [-5, 3, 3], 3, 5) == 0


def test_stroke_from_picks():
    v = [np.array(c) for c in ((1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4), (5, 5, 5))]
    pts, seg = sm.stroke_from_picks([v[0], v[1], None, v[2], None, None, v[3], v[4], None])
    assert pts.tolist() == [list(c) for c in v] and seg.tolist() == [[0, 1], [3, 4], [2, 2]]
    pts, seg = sm.stroke_from_picks([None, None])
    assert pts.shape == (0, 3) and seg.shape == (0, 2)
    pts, seg = sm.stroke_from_picks([v[0]])
    assert seg.tolist() == [[0, 0]]
