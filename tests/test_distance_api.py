"""Exact Euclidean distance without a GPU: the entry points are exported and bound, the Python tdt_round layout is the header's,
the kernels of tdt_distance.hip cross-compile without scratch or spills, the wrapper checks its arguments, and the numpy model
the GPU tests compare against (tests/distance_model.py) equals the all-pairs brute force in distances AND nearest voxels,
scipy's transform, one step of the step-wise morphology model at squared radius 1 and 3, and the ops' own identities.  The
unit itself, compiled for the CPU, runs against the definitions under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import distance_model as dm
import morph_model as mm
from test_gpu_region_edit import brush_voxels, sort_vox
from tdt4230_project_raytracing_amd import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_octree_morph_round", "tdt_octree_extract_morph_round", "tdt_octree_distance_field")
OPS = (dm.DILATE, dm.ERODE, dm.OPEN, dm.CLOSE, dm.SHELL)


def random_list(depth, density, seed):
    rng = np.random.default_rng(seed)
    n = 1 << depth
    p = np.argwhere(rng.random((n, n, n)) < density)
    return sort_vox(np.concatenate([p, rng.integers(1, 255, (len(p), 1))], 1))


def test_distance_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    for n in ("octree_morph_round", "octree_extract_morph_round", "octree_distance_field"):
        assert callable(getattr(rt.Context, n)), n


def test_round_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_round \{(.*?)\} tdt_round;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"int32_t\s+(\w+);", body)
    assert fields == [f[0] for f in rt.Round._fields_] == ["op", "radius2", "material", "border"]
    for i, name in enumerate(fields):
        assert getattr(rt.Round, name).offset == 4 * i and dict(rt.Round._fields_)[name] is ctypes.c_int32
    assert ctypes.sizeof(rt.Round) == 16
    assert len(re.findall(r"sizeof\(tdt_round\) == 16", text)) == 2          # C++ and C
    assert int(re.search(r"#define TDT_ROUND_DOMAIN_CAP \(1u << (\d+)\)", text).group(1)) == 28 and rt.ROUND_DOMAIN_CAP == 1 << 28


def test_distance_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_distance.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"dist_pass_x_kernel", "dist_scan_kernel", "dist_count_kernel", "dist_emit_kernel"} <= names     # the shared steps: test_bitvol_api.py
    assert sum("dist_scan_kernel<" in r["name"] for r in rows) == 3          # pass y, pass z into bits, pass z into the field
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


def test_python_wrapper_argument_checks():
    r = rt.Context._round(rt.MORPH_CLOSE, 5, None, 1)
    assert (r.op, r.radius2, r.material, r.border) == (rt.MORPH_CLOSE, 5, -1, 1)
    assert rt.Context._round(0, 4096, 253, True).border == 1
    assert rt.Context._round(9, 0, 999, 7).radius2 == 0                      # the ranges are the library's to check
    for bad in (lambda: rt.Context._round(True, 1, 0, 0), lambda: rt.Context._round(0, True, 0, 0), lambda: rt.Context._round(0, 1, False, 0),
                lambda: rt.Context._round(0, 2.5, 0, 0), lambda: rt.Context._round(0, 1, 1.5, 0), lambda: rt.Context._round(0, 2 ** 31, 0, 0),
                lambda: rt.Context._round(0, 1, 0, -2 ** 31 - 1), lambda: rt.Context._round(0.5, 1, 0, 0)):
        with pytest.raises(ValueError):
            bad()
    # the field's arguments are checked before the library (or a context) is touched
    c = object.__new__(rt.Context)
    for bad in (lambda: c.octree_distance_field((0, 0), (1, 1, 1), 4), lambda: c.octree_distance_field((0, 0, 0), (1, 1.5, 1), 4),
                lambda: c.octree_distance_field((0, 0, 0), (1, 1, 2 ** 31), 4), lambda: c.octree_distance_field((0, 0, True), (1, 1, 1), 4),
                lambda: c.octree_distance_field((0, 0, 0), (1, 1, 1), 4.5), lambda: c.octree_distance_field((0, 0, 0), (1, 1, 1), True),
                lambda: c.octree_distance_field((0, 0, 0), (1, 1, 1), 4, border=0.5)):
        with pytest.raises(ValueError):
            bad()


# ---- the model against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,density", [(3, 0.1), (3, 0.5), (4, 0.02), (4, 0.3)])
def test_model_equals_the_all_pairs_brute_force(depth, density):
    n = 1 << depth
    occ = np.random.default_rng(depth * 100 + int(density * 100)).random((n, n, n)) < density
    assert dm.SPARSE < occ.sum() < n ** 3
    assert dm.ties(occ) > n                                                 # tied nearest voxels exist: the rank half of the key is exercised
    want = dm.brute(occ)
    got = dm.transform(occ)
    assert np.array_equal(got, want)                                         # distances and nearest voxels in one key
    d2 = dm.split(want)[0]
    for R in (1, 2, 3):                                                      # the capped window is exact wherever d2 <= R^2
        capped = dm.transform(occ, R)
        assert np.array_equal(capped[d2 <= R * R], want[d2 <= R * R]) and (dm.split(capped)[0][d2 > R * R] > R * R).all()
    few = np.zeros_like(occ)
    few.reshape(-1)[np.flatnonzero(occ)[: dm.SPARSE]] = True                 # the all-pairs form of sparse sets
    assert np.array_equal(dm.transform(few), dm.brute(few)) and dm.ties(few) > 0


def test_model_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for depth, density in ((4, 0.05), (5, 0.01), (5, 0.4)):
        n = 1 << depth
        occ = np.random.default_rng(depth).random((n, n, n)) < density
        want = np.rint(ndi.distance_transform_edt(~occ) ** 2).astype(np.int64)
        assert np.array_equal(dm.split(dm.transform(occ))[0], want)


@pytest.mark.parametrize("depth,density", [(3, 0.15), (4, 0.1), (5, 0.05)])
def test_radius2_one_and_three_are_single_steps_of_the_step_model(depth, density):
    V = random_list(depth, density, depth)
    for material in (None, 9):
        assert np.array_equal(dm.round_op(V, depth, dm.DILATE, 1, material), mm.morph(V, depth, mm.DILATE, 1, 6, material))
    got, want = dm.round_op(V, depth, dm.DILATE, 3), mm.morph(V, depth, mm.DILATE, 1, 26)
    assert np.array_equal(got[:, :3], want[:, :3]) and not np.array_equal(got[:, 3], want[:, 3])    # inherited materials differ, by design
    assert np.array_equal(dm.round_op(V, depth, dm.DILATE, 3, 9), mm.morph(V, depth, mm.DILATE, 1, 26, 9))
    D = random_list(depth, 0.85, depth + 50)
    for border in (0, 1):
        for op in (dm.ERODE, dm.SHELL):
            assert np.array_equal(dm.round_op(D, depth, op, 1, border=border), mm.morph(D, depth, op, 1, 6, border=border))
            assert np.array_equal(dm.round_op(D, depth, op, 3, border=border), mm.morph(D, depth, op, 1, 26, border=border))


@pytest.mark.parametrize("radius2", [1, 2, 5, 9])
def test_erode_is_the_complement_of_the_dilated_complement(radius2):
    depth, n = 4, 16
    mat = dm.grid_of(random_list(depth, 0.8, radius2), depth)
    # border 1: the complement inside the grid alone
    comp = np.where(mat > 0, 0, 1).astype(np.int32)
    assert np.array_equal(dm.erode(mat, radius2, 1) > 0, dm.dilate(comp, radius2, 0) == 0)
    # border 0: the same on a grid padded with empty space all round, cut back
    R = dm.window_of(radius2)
    big = np.ones((n + 2 * R,) * 3, np.int32)
    big[R:-R, R:-R, R:-R] = comp
    inner = (slice(R, -R),) * 3
    assert np.array_equal(dm.erode(mat, radius2, 0) > 0, dm.dilate(big, radius2, 0)[inner] == 0)
    assert 0 < (dm.erode(mat, radius2, 0) > 0).sum() < (dm.erode(mat, radius2, 1) > 0).sum() or radius2 > 2


@pytest.mark.parametrize("radius2", [1, 3, 4, 8])
def test_open_and_close_are_ordered_and_idempotent(radius2):
    depth = 4
    V = random_list(depth, 0.55, radius2)
    keys = lambda L: set(map(tuple, L[:, :3]))                               # noqa: E731
    O, C = dm.round_op(V, depth, dm.OPEN, radius2), dm.round_op(V, depth, dm.CLOSE, radius2)
    assert keys(O) <= keys(V) <= keys(C) and (len(O) < len(V) or len(V) < len(C))
    assert np.array_equal(O, V[np.isin(mm._keys(V[:, :3]), mm._keys(O[:, :3]))])          # V's own materials
    assert np.array_equal(dm.round_op(O, depth, dm.OPEN, radius2), O)
    assert np.array_equal(dm.round_op(C, depth, dm.CLOSE, radius2), C)


@pytest.mark.parametrize("r", [1, 2, 3, 5])
def test_one_voxel_dilated_is_the_sphere_brush(r):
    depth, c = 4, (6, 9, 3)                                                  # clipped by the grid at z = 0 for r > 3
    got = dm.round_op(np.array([[*c, 41]], np.int32), depth, dm.DILATE, r * r)
    want = brush_voxels([rt.sphere(c, r)], depth)
    assert set(map(tuple, got[:, :3])) == set(map(tuple, want)) and set(got[:, 3]) == {41}


def test_field_of_the_model_by_hand():
    V = np.array([[2, 2, 2, 7], [3, 2, 2, 8]], np.int32)
    f, near = dm.field(V, 3, (0, 2, 2), (7, 2, 2), 4)
    assert f.shape == (1, 1, 8) and near.shape == (1, 1, 8, 3)
    assert f[0, 0].tolist() == [4, 1, -1, -1, 1, 4, 5, 5]
    assert near[0, 0].tolist() == [[2, 2, 2], [2, 2, 2], [2, 2, 2], [3, 2, 2], [3, 2, 2], [3, 2, 2], [-1, -1, -1], [-1, -1, -1]]
    full = np.concatenate([np.argwhere(np.ones((8, 8, 8), bool)), np.ones((512, 1), int)], 1)
    assert dm.field(full, 3, (0, 0, 0), (7, 7, 7), 9, border=0)[0][3, 3, :].tolist() == [-1, -4, -9, -10, -10, -9, -4, -1]
    assert (dm.field(full, 3, (0, 0, 0), (7, 7, 7), 9, border=1)[0] == -10).all()


def test_the_unit_compiled_for_the_cpu_runs_clean_under_the_sanitizers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostsim", "run.py"), "distance"], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout and "MISMATCH" not in r.stdout and "ERROR" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
