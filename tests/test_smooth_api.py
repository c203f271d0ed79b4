"""Voxel smoothing without a GPU: the entry points are exported and bound, the Python tdt_smooth layout is the header's,
tdt_ball_size counts the ball, the kernels of tdt_smooth.hip cross-compile without scratch or spills, the wrapper checks its
arguments, and the numpy model the GPU tests compare against (tests/smooth_model.py) equals a literal loop over every offset of
the ball and satisfies the header's identities against tests/distance_model.py.  The unit itself, compiled for the CPU, runs
against its own brute force under AddressSanitizer and UBSan."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import distance_model as dm
import smooth_model as sm
from test_gpu_region_edit import sort_vox
from tdt4230_project_raytracing_amd import build, rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_ball_size", "tdt_octree_smooth", "tdt_octree_extract_smooth", "tdt_octree_density_field")
MODES = (sm.BOTH, sm.ADD, sm.REMOVE)


def random_grid(depth, density, seed):
    """material + 1 on an [x, y, z] grid."""
    rng = np.random.default_rng(seed)
    n = 1 << depth
    return np.where(rng.random((n, n, n)) < density, rng.integers(1, 255, (n, n, n)), 0).astype(np.int32)


def test_smooth_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    for n in ("octree_smooth", "octree_extract_smooth", "octree_density_field"):
        assert callable(getattr(rt.Context, n)), n
    assert callable(rt.ball_size) and "tdt_smooth.hip" in build.DEVICE_UNITS


def test_smooth_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_smooth \{(.*?)\} tdt_smooth;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"int32_t\s+(\w+);", body)
    assert fields == [f[0] for f in rt.Smooth._fields_] == ["radius2", "iterations", "threshold", "mode", "material", "border"]
    for i, name in enumerate(fields):
        assert getattr(rt.Smooth, name).offset == 4 * i and dict(rt.Smooth._fields_)[name] is ctypes.c_int32
    assert ctypes.sizeof(rt.Smooth) == 24
    assert len(re.findall(r"sizeof\(tdt_smooth\) == 24", text)) == 2         # C++ and C
    assert int(re.search(r"#define TDT_SMOOTH_DOMAIN_CAP \(1u << (\d+)\)", text).group(1)) == 28 and rt.SMOOTH_DOMAIN_CAP == 1 << 28
    modes = re.search(r"enum \{ TDT_SMOOTH_BOTH = (\d), TDT_SMOOTH_ADD = (\d), TDT_SMOOTH_REMOVE = (\d) \};", text).groups()
    assert tuple(map(int, modes)) == (rt.SMOOTH_BOTH, rt.SMOOTH_ADD, rt.SMOOTH_REMOVE) == (0, 1, 2)


def test_ball_size_is_a_literal_count_and_odd():
    ax = np.arange(-15, 16)
    d2 = (ax ** 2)[:, None, None] + (ax ** 2)[None, :, None] + (ax ** 2)[None, None, :]
    for r2 in range(1, 226):
        want = int((d2 <= r2).sum())
        assert rt.ball_size(r2) == want == sm.ball_size(r2) and want % 2 == 1, r2
        assert max(h for _, _, h in sm.chords(r2)) <= 15                     # every x-chord at most 31 wide
    assert rt.ball_size(225) < 1 << 15                                      # the threshold test fits 32 unsigned bits
    assert rt.ball_size(4096) == int(sum(2 * int(np.sqrt(4096 - a * a - b * b)) + 1 for a in range(-64, 65) for b in range(-64, 65) if a * a + b * b <= 4096))
    for bad in (0, -1, 4097, 2 ** 31 - 1):
        assert rt.ball_size(bad) == -1
    for bad in (True, 1.5, 2 ** 31):
        with pytest.raises(ValueError):
            rt.ball_size(bad)


def test_smooth_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_smooth.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"smooth_density_kernel", "smooth_count_kernel", "smooth_emit_kernel", "smooth_inherit_kernel"} <= names   # the shared steps: test_bitvol_api.py
    assert sum("smooth_density_kernel<" in r["name"] for r in rows) == 2     # the step and the field
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]
        assert r["LDS Size [bytes/block]"] <= 64 * 1024, r["name"]


def test_python_wrapper_argument_checks():
    s = rt.Context._smooth(5, 2, None, rt.SMOOTH_ADD, None, 1)
    assert (s.radius2, s.iterations, s.threshold, s.mode, s.material, s.border) == (5, 2, 0, rt.SMOOTH_ADD, -1, 1)
    assert rt.Context._smooth(225, 16, 65536, 2, 253, True).border == 1
    assert rt.Context._smooth(0, 99, -5, 9, 999, 7).iterations == 99         # the ranges are the library's to check
    S = rt.Context._smooth
    for bad in (lambda: S(True, 1, 0, 0, 0, 0), lambda: S(1, True, 0, 0, 0, 0), lambda: S(1, 1, False, 0, 0, 0), lambda: S(1, 1, 0, True, 0, 0),
                lambda: S(1, 1, 0, 0, False, 0), lambda: S(2.5, 1, 0, 0, 0, 0), lambda: S(1, 1.5, 0, 0, 0, 0), lambda: S(1, 1, 0.5, 0, 0, 0),
                lambda: S(1, 1, 0, 0, 0, 0.5), lambda: S(2 ** 31, 1, 0, 0, 0, 0), lambda: S(1, 1, 0, 0, 0, -2 ** 31 - 1)):
        with pytest.raises(ValueError):
            bad()
    # the arguments are checked before the library (or a context) is touched
    c = object.__new__(rt.Context)
    for bad in (lambda: c.octree_smooth(2.5), lambda: c.octree_extract_smooth(3, iterations=True), lambda: c.octree_smooth(3, threshold=0.5),
                lambda: c.octree_density_field((0, 0), (1, 1, 1), 4), lambda: c.octree_density_field((0, 0, 0), (1, 1.5, 1), 4),
                lambda: c.octree_density_field((0, 0, 0), (1, 1, 2 ** 31), 4), lambda: c.octree_density_field((0, 0, True), (1, 1, 1), 4),
                lambda: c.octree_density_field((0, 0, 0), (1, 1, 1), 4.5), lambda: c.octree_density_field((0, 0, 0), (1, 1, 1), True)):
        with pytest.raises(ValueError):
            bad()


# ---- the model against the definition ------------------------------------------------------------------------------------------
def brute_counts(occ, r2):
    """(density, support) by a loop over every d in B on an array padded by R: the definition itself."""
    n = occ.shape[0]
    R = dm.window_of(r2)
    pad = np.zeros((n + 2 * R,) * 3, np.int32)
    pad[R:R + n, R:R + n, R:R + n] = occ
    grid = np.zeros_like(pad)
    grid[R:R + n, R:R + n, R:R + n] = 1
    d, s = np.zeros((n, n, n), np.int32), np.zeros((n, n, n), np.int32)
    for dx, dy, dz in itertools.product(range(-R, R + 1), repeat=3):
        if dx * dx + dy * dy + dz * dz <= r2:
            w = (slice(R + dx, R + dx + n), slice(R + dy, R + dy + n), slice(R + dz, R + dz + n))
            d += pad[w]
            s += grid[w]
    return d, s


def brute_step(occ, d, s, r2, threshold, mode, border):
    """The occupancy after one step, from the literal counts (d, s)."""
    n = s.astype(np.int64) if border else np.int64(len(sm.offsets(r2)))
    t = 2 * d.astype(np.int64) > n if threshold == 0 else 65536 * d.astype(np.int64) >= threshold * n
    return t if mode == sm.BOTH else (occ | t) if mode == sm.ADD else (occ & t)


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("depth,radii2", [(3, (1, 3, 6, 225)), (4, (2, 5, 16))])
def test_model_equals_the_all_offsets_brute_force(depth, radii2, density):
    mat = random_grid(depth, density, depth * 100 + int(density * 10))
    occ = mat > 0
    n = 1 << depth
    for r2 in radii2:
        d, s = brute_counts(occ, r2)
        assert np.array_equal(sm.density(occ, r2), d) and np.array_equal(sm.support(n, r2), s), r2
        assert s.max() == sm.ball_size(r2) or dm.window_of(r2) * 2 >= n
        for border, threshold, mode in itertools.product((0, 1), (0, 1, 20000, 65536), MODES):
            got = sm.step(mat, r2, threshold, mode, 7, border)
            assert np.array_equal(got > 0, brute_step(occ, d, s, r2, threshold, mode, border)), (r2, border, threshold, mode)
            assert np.array_equal(got[occ & (got > 0)], mat[occ & (got > 0)]) and (got[~occ & (got > 0)] == 8).all()
    f, sup = sm.field(dm.list_of(mat), depth, (1, 0, 2), (n - 2, n - 1, 2), radii2[1])
    d, s = brute_counts(occ, radii2[1])
    assert f.shape == (1, n, n - 2) and np.array_equal(f, d[1:n - 1, :, 2:3].transpose(2, 1, 0)) and np.array_equal(sup, s[1:n - 1, :, 2:3].transpose(2, 1, 0))


# ---- the identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,density", [(3, 0.15), (4, 0.1), (5, 0.3)])
def test_threshold_one_is_the_round_dilate_and_the_full_threshold_the_round_erode(depth, density):
    V = dm.list_of(random_grid(depth, density, depth))
    D = dm.list_of(random_grid(depth, 0.9, depth + 50))
    for r2 in (1, 3, 5, 16):
        for material in (None, 9):
            assert np.array_equal(sm.smooth(V, depth, r2, threshold=1, material=material), dm.round_op(V, depth, dm.DILATE, r2, material)), (r2, material)
        for border in (0, 1):
            assert np.array_equal(sm.smooth(D, depth, r2, threshold=65536, border=border), dm.round_op(D, depth, dm.ERODE, r2, border=border)), (r2, border)


def test_a_few_voxels_far_apart_inherit_like_the_round_dilate():
    """The model's all-pairs form of the nearest voxel (sparse sets), ties included."""
    depth, rng = 5, np.random.default_rng(3)
    p = rng.integers(8, 24, (12, 3))
    p[1], p[3] = p[0] + (2, 0, 0), p[2] + (1, 2, 0) - (2, 1, 0)               # an axis tie and a diagonal tie
    V = sort_vox(np.concatenate([np.unique(p, axis=0), np.arange(1, 1 + len(np.unique(p, axis=0)))[:, None]], 1))
    assert len(V) <= sm.SPARSE and dm.sparse_ties(V, depth) > 0
    for r2 in (5, 30, 100):
        assert np.array_equal(sm.smooth(V, depth, r2, threshold=1), dm.round_op(V, depth, dm.DILATE, r2)), r2


@pytest.mark.parametrize("r2", [2, 6, 30])
def test_inherited_materials_are_the_nearest_voxel_of_distance_model(r2):
    depth = 4
    mat = random_grid(depth, 0.35, r2)
    for threshold, mode in ((0, sm.BOTH), (20000, sm.ADD), (9000, sm.BOTH)):
        got = sm.step(mat, r2, threshold, mode, None, 0)
        new = (got > 0) & (mat == 0)
        assert new.sum() > 10 or (threshold == 0 and r2 > 2)                 # (a majority of a large ball is out of a 35 % grid's reach)
        d2, rank, found = dm.split(dm.transform(mat > 0))
        assert found[new].all() and (d2[new] <= r2).all()                    # T implies d >= 1
        assert np.array_equal(got[new], mat.reshape(-1)[rank[new]])
    assert dm.ties(mat > 0) > 16                                              # tied nearest voxels exist: the order is exercised


@pytest.mark.parametrize("r2", [1, 4, 11])
def test_add_is_a_superset_and_remove_a_subset(r2):
    depth = 4
    mat = random_grid(depth, 0.5, r2)
    for threshold, border, iterations in itertools.product((0, 20000, 50000), (0, 1), (1, 3)):
        add = sm.smooth_grid(mat, r2, iterations, threshold, sm.ADD, None, border)
        rem = sm.smooth_grid(mat, r2, iterations, threshold, sm.REMOVE, None, border)
        assert ((add > 0) >= (mat > 0)).all() and np.array_equal(add[mat > 0], mat[mat > 0])
        assert ((rem > 0) <= (mat > 0)).all() and np.array_equal(rem[rem > 0], mat[rem > 0])
        both = sm.smooth_grid(mat, r2, 1, threshold, sm.BOTH, None, border)
        assert np.array_equal(sm.smooth_grid(mat, r2, 1, threshold, sm.ADD, None, border) > 0, (mat > 0) | (both > 0))
        assert np.array_equal(sm.smooth_grid(mat, r2, 1, threshold, sm.REMOVE, None, border) > 0, (mat > 0) & (both > 0))


@pytest.mark.parametrize("r2", [1, 3, 9, 40, 225])
def test_a_majority_step_with_an_empty_outside_stays_inside_the_bounding_box(r2):
    depth, n = 4, 16
    mat = np.zeros((n, n, n), np.int32)
    mat[3:11, 5:9, 2:14] = random_grid(depth, 0.97, r2)[3:11, 5:9, 2:14]     # a nearly solid box: the best case for growing out of it
    mat[3, 5, 2] = mat[10, 8, 13] = 4
    for threshold in (0, 32769, 65536):
        out = sm.step(mat, r2, threshold, sm.ADD, 1, 0)
        p = np.argwhere(out > 0)
        assert (p.min(0) >= (3, 5, 2)).all() and (p.max(0) <= (10, 8, 13)).all(), (r2, threshold)


def test_a_slab_cut_by_a_grid_face_is_a_fixed_point_only_with_the_outside_left_out():
    depth, n = 4, 16
    mat = np.zeros((n, n, n), np.int32)
    mat[:, :, :6] = 5                                                         # a flat slab through the whole grid, cut by five faces
    for r2 in (3, 9):
        assert np.array_equal(sm.smooth_grid(mat, r2, 3, border=1), mat)
        cut = sm.smooth_grid(mat, r2, 3, border=0)
        assert not np.array_equal(cut, mat) and ((cut > 0) <= (mat > 0)).all() and cut[0, 0, 0] == 0 and cut[8, 8, 2] == 5


def test_a_single_voxel_vanishes_under_majority():
    V = np.array([[5, 6, 7, 9]], np.int32)
    for r2, border in itertools.product((1, 2, 225), (0, 1)):
        assert len(sm.smooth(V, 4, r2, border=border)) == 0
    assert np.array_equal(sm.smooth(V, 4, 1, mode=sm.ADD), V)
    assert len(sm.smooth(V, 4, 1, threshold=1)) == 7
    assert np.array_equal(sort_vox(V), V)


def test_the_unit_compiled_for_the_cpu_runs_clean_under_the_sanitizers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostsim", "run.py"), "smooth"], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout and "MISMATCH" not in r.stdout and "ERROR" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
