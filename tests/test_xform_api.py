"""Affine transforms of voxel selections without a GPU: the entry points are exported and bound, the Python tdt_xform layout is the
header's, the kernels of tdt_xform.hip cross-compile without scratch or spills, the wrapper checks its arguments, the numpy
model the GPU tests compare against (tests/xform_model.py) satisfies the identities the definition was chosen for (identity,
array shifts, numpy.rot90 on every axis, mirrors, numpy.kron, point sampling), the builders of libtdthost.so produce exactly the
documented integers, and the unit itself, compiled for the CPU, runs against a brute force under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import xform_model as xm
from distance_model import grid_of, list_of
from test_gpu_region_edit import sort_vox
from tdt4230_project_raytracing_amd import host, rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_octree_transform", "tdt_octree_extract_transform", "tdt_debug_xform_bricks")
HOST_NAMES = ("tdt_xform_identity", "tdt_xform_translate", "tdt_xform_quarter_turns", "tdt_xform_mirror", "tdt_xform_scale",
              "tdt_xform_from_affine", "tdt_xform_rotate")


def random_list(depth, density, seed):
    rng = np.random.default_rng(seed)
    n = 1 << depth
    p = np.argwhere(rng.random((n, n, n)) < density)
    return sort_vox(np.concatenate([p, rng.integers(1, 255, (len(p), 1))], 1))


def same_fields(got, want):
    """An rt.Xform from the library against an xform_model.X."""
    return (list(got.a) == want.a and list(got.t) == want.t and got.material == -1 and list(got.dst_lo) == [0, 0, 0]
            and list(got.dst_hi) == [2 ** 31 - 1] * 3 and list(got.pad) == [0, 0])


def test_transform_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    for n in ("octree_transform", "octree_extract_transform", "xform_bricks"):
        assert callable(getattr(rt.Context, n)), n
    H = host.lib()
    text = open(os.path.join(ROOT, "include", "tdt_host.h")).read()
    for n in HOST_NAMES:
        assert hasattr(H, n) and re.search(r"\bint " + n + r"\(", text), n
        assert callable(getattr(host, n[4:])), n
    assert "EQUAL PARITY" in text                               # when a quarter turn is a bijection


def test_xform_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_xform \{(.*?)\} tdt_xform;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, decl in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body):
        for name, count in re.findall(r"(\w+)(?:\[(\d+)\])?", decl):
            fields.append((name, ctype, int(count or 1)))
    assert fields == [("t", "int64_t", 3), ("a", "int32_t", 9), ("material", "int32_t", 1), ("dst_lo", "int32_t", 3),
                      ("dst_hi", "int32_t", 3), ("pad", "int32_t", 2)]
    assert [f[0] for f in rt.Xform._fields_] == [f[0] for f in fields]
    offset = 0
    for name, ctype, count in fields:
        size = 8 if ctype == "int64_t" else 4
        assert getattr(rt.Xform, name).offset == offset and getattr(rt.Xform, name).size == size * count, name
        offset += size * count
    assert offset == ctypes.sizeof(rt.Xform) == 96
    assert len(re.findall(r"sizeof\(tdt_xform\) == 96", text)) == 2          # C++ and C
    assert int(re.search(r"#define TDT_XFORM_ONE (\d+)", text).group(1)) == rt.XFORM_ONE == xm.ONE == 65536


def test_xform_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_xform.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"xform_brick_kernel", "xform_count_kernel", "xform_emit_kernel"} <= names      # the shared steps: test_bitvol_api.py
    assert not {n for n in names if n.startswith("bitvol_")}                              # which has the bit volume's kernels to itself
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


def test_python_wrapper_argument_checks():
    x = rt.Context._xform(dict(a=range(9), t=(1, -2 ** 40, 2 ** 62), material=None, dst_lo=(3, 3, 3), dst_hi=(12, 2, 12)))
    assert list(x.a) == list(range(9)) and list(x.t) == [1, -2 ** 40, 2 ** 62] and x.material == -1
    assert list(x.dst_lo) == [3, 3, 3] and list(x.dst_hi) == [12, 2, 12] and list(x.pad) == [0, 0]
    d = rt.Context._xform({})
    assert list(d.a) == [65536, 0, 0, 0, 65536, 0, 0, 0, 65536] and list(d.t) == [0, 0, 0] and list(d.dst_hi) == [2 ** 31 - 1] * 3
    y = rt.Context._xform(x)
    assert y is not x and bytes(y) == bytes(x)
    assert rt.Context._xform(dict(material=999, a=[2 ** 31 - 1] * 9)).material == 999    # the ranges are the library's to check
    for bad in (dict(a=range(8)), dict(t=(0, 0)), dict(a=[0.5] * 9), dict(a=[2 ** 31] * 9), dict(t=(0, 0, 2 ** 63)), dict(t=(True, 0, 0)),
                dict(material=1.5), dict(material=True), dict(dst_lo=(0, 0)), dict(dst_hi=(0, 0, 2 ** 31)), dict(pad=(0,)), [1, 2, 3], None):
        with pytest.raises(ValueError):
            rt.Context._xform(bad)
    c = object.__new__(rt.Context)                               # checked before the library (or a context) is touched
    for bad in (lambda: c.octree_transform(dict(a=range(3))), lambda: c.octree_transform({}, op=1.5), lambda: c.octree_transform({}, op=True),
                lambda: c.octree_extract_transform("turn")):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: host.xform_translate((1, 2)), lambda: host.xform_translate((1, 2, 2.5)), lambda: host.xform_translate((1, 2, 2 ** 24)),
                lambda: host.xform_quarter_turns(3, 1, (0, 0, 0)), lambda: host.xform_mirror(-1, (0, 0, 0)),
                lambda: host.xform_scale((1, 1, 0), (1, 1, 1), (0, 0, 0)), lambda: host.xform_scale((1, 1, 1), (17, 1, 1), (0, 0, 0)),
                lambda: host.xform_scale((1, 1, 1), (1, 1, 1), (0, 0)), lambda: host.xform_from_affine(np.zeros((3, 4))),
                lambda: host.xform_from_affine(np.eye(3)), lambda: host.xform_from_affine([[1e-3, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]),
                lambda: host.xform_from_affine([[1, 0, 0, 1e9], [0, 1, 0, 0], [0, 0, 1, 0]]), lambda: host.xform_rotate((0, 0, 0), 30, (1, 1, 1)),
                lambda: host.xform_quarter_turns(2, 1, (2 ** 25, -2 ** 25, 0))):
        with pytest.raises(ValueError):
            bad()


# ---- the model against the identities of the definition ------------------------------------------------------------------------
DEPTH, N = 4, 16


@pytest.fixture(scope="module")
def V():
    v = random_list(DEPTH, 0.3, 4)
    v = v[~((v[:, :3] == 0).any(1))]
    return sort_vox(np.concatenate([v, [[0, 5, 9, 200], [3, 0, 0, 201], [15, 15, 0, 202]]]))      # voxels at coordinate 0 for sure


def test_model_identity_and_shift(V):
    assert np.array_equal(xm.transform(V, DEPTH, xm.identity()), V)
    g = grid_of(V, DEPTH)
    for d in ((1, 0, 0), (1, -3, 5), (-N + 1, 0, 0), (0, N - 1, 0)):
        want = np.zeros_like(g)
        src = tuple(slice(max(-k, 0), N - max(k, 0)) for k in d)
        dst = tuple(slice(max(k, 0), N - max(-k, 0)) for k in d)
        want[dst] = g[src]
        got = xm.transform(V, DEPTH, xm.translate(d))
        assert np.array_equal(got, list_of(want)) and 0 < len(got) < len(V), d
    one = np.array([[0, 7, 7, 9]], np.int32)                     # a truncating divide would leave a copy behind at x = 0
    assert xm.transform(one, DEPTH, xm.translate((1, 0, 0))).tolist() == [[1, 7, 7, 9]]
    assert xm.transform(one, DEPTH, xm.translate((-1, 0, 0))).tolist() == []


def test_model_quarter_turns_are_rot90(V):
    g = grid_of(V, DEPTH)
    for axis in range(3):
        axes = ((axis + 1) % 3, (axis + 2) % 3)
        cur = V
        for k in range(1, 5):
            want = list_of(np.rot90(g, k, axes=axes))
            assert np.array_equal(xm.transform(V, DEPTH, xm.quarter_turns(axis, k, (N, N, N))), want), (axis, k)
            cur = xm.transform(cur, DEPTH, xm.quarter_turns(axis, 1, (N, N, N)))
            assert np.array_equal(cur, want), (axis, k)
        assert np.array_equal(cur, V)                            # four turns
        assert not np.array_equal(xm.transform(V, DEPTH, xm.quarter_turns(axis, 1, (N, N, N))), V)
    assert xm.quarter_turns(2, 1, (N, N, N)).a == [0, 65536, 0, -65536, 0, 0, 0, 0, 65536]
    assert xm.quarter_turns(2, 1, (N, N, N)).t == [0, 65536 * 2 * N, 0]    # 65536 (P - R^-1 P)
    # an off-centre pivot with equal parity is a bijection of the lattice: nothing is lost but what leaves the grid
    inner = V[((V[:, :3] >= 4) & (V[:, :3] < 12)).all(1)]
    turned = xm.transform(inner, DEPTH, xm.quarter_turns(2, 1, (15, 17, 0)))
    assert len(turned) == len(inner) and np.array_equal(xm.transform(turned, DEPTH, xm.quarter_turns(2, -1, (15, 17, 0))), inner)


def test_model_mirror_twice_is_the_identity(V):
    g = grid_of(V, DEPTH)
    for axis in range(3):
        m = xm.mirror(axis, (N, N, N))
        once = xm.transform(V, DEPTH, m)
        assert np.array_equal(once, list_of(np.flip(g, axis))) and not np.array_equal(once, V)
        assert np.array_equal(xm.transform(once, DEPTH, m), V)


def test_model_scale_is_kron_and_point_sampling(V):
    g = grid_of(V, DEPTH)
    double = xm.scale((2, 2, 2), (1, 1, 1), (0, 0, 0))
    assert double.a == [32768, 0, 0, 0, 32768, 0, 0, 0, 32768] and double.t == [0, 0, 0]
    want = np.kron(g, np.ones((2, 2, 2), g.dtype))[:N, :N, :N]
    assert np.array_equal(xm.transform(V, DEPTH, double), list_of(want)) and want.any()
    half = xm.scale((1, 1, 1), (2, 2, 2), (0, 0, 0))
    assert half.a[0] == 131072 and half.t == [0, 0, 0]
    want = np.zeros_like(g)
    want[: N // 2, : N // 2, : N // 2] = g[1::2, 1::2, 1::2]   # (2 (2 p + 1)) >> 1 = 2 p + 1: the odd voxels
    assert np.array_equal(xm.transform(V, DEPTH, half), list_of(want)) and want.any()


def test_model_material_mask_and_dst(V):
    x = xm.translate((2, 0, -1))
    fixed = xm.transform(V, DEPTH, x.with_(material=0))
    plain = xm.transform(V, DEPTH, x)
    assert np.array_equal(fixed[:, :3], plain[:, :3]) and set(fixed[:, 3]) == {1} and len(set(plain[:, 3])) > 1
    mask = [rt.box((1, 0, 2), (8, 14, 15)), rt.sphere((8, 8, 5), 5)]
    from test_gpu_region_edit import inside
    sel = V[inside(V[:, :3], mask)]
    assert 0 < len(sel) < len(V)
    assert np.array_equal(xm.transform(V, DEPTH, x, mask), xm.transform(sel, DEPTH, x))
    assert len(xm.transform(V, DEPTH, x, [])) == 0
    cut = xm.transform(V, DEPTH, x.with_(dst_lo=[3, 0, -5], dst_hi=[12, 99, 15]))
    assert np.array_equal(cut, plain[(plain[:, 0] >= 3) & (plain[:, 0] <= 12)]) and 0 < len(cut) < len(plain)
    assert len(xm.transform(V, DEPTH, x.with_(dst_lo=[5, 0, 0], dst_hi=[4, 15, 15]))) == 0


# ---- the builders of libtdthost.so -----------------------------------------------------------------------------------------------
PIVOTS = ((16, 16, 16), (15, 17, 3), (-7, 40, 1001), (0, 0, 0))


def affine_of(rinv_q16, pivot2):
    """The forward map [F | f] on continuous coordinates whose inverse matrix is rinv_q16 / 65536 (exact in doubles here) about
    the doubled point pivot2: x' = F (x - c) + c, c = pivot2 / 2."""
    F = np.linalg.inv(np.array(rinv_q16, np.float64).reshape(3, 3) / 65536.0)
    c = np.array(pivot2, np.float64) / 2
    return np.concatenate([F, (c - F @ c)[:, None]], 1)


def test_integer_builders_are_the_documented_closed_forms():
    assert same_fields(host.xform_identity(), xm.identity())
    for d in ((1, -3, 5), (-1023, 0, 0), (2 ** 23, -2 ** 23, 7)):
        assert same_fields(host.xform_translate(d), xm.translate(d)), d
        f = np.concatenate([np.eye(3), np.array(d, np.float64)[:, None]], 1)
        assert same_fields(host.xform_from_affine(f), xm.translate(d)), d
    for p in PIVOTS:
        for axis in range(3):
            for k in range(-1, 6):
                want = xm.quarter_turns(axis, k, p)
                assert same_fields(host.xform_quarter_turns(axis, k, p), want), (axis, k, p)
                assert same_fields(host.xform_from_affine(affine_of(want.a, p)), want), (axis, k, p)
            want = xm.mirror(axis, p)
            assert same_fields(host.xform_mirror(axis, p), want), (axis, p)
            assert same_fields(host.xform_from_affine(affine_of(want.a, p)), want), (axis, p)
        for num, den in (((2, 2, 2), (1, 1, 1)), ((1, 1, 1), (2, 2, 2)), ((4, 1, 2), (1, 8, 1)), ((1, 1, 1), (16, 16, 16))):
            want = xm.scale(num, den, p)
            assert same_fields(host.xform_scale(num, den, p), want), (num, den, p)
            assert same_fields(host.xform_from_affine(affine_of(want.a, p)), want), (num, den, p)     # powers of two: exact doubles
        want = xm.scale((3, 3, 3), (2, 2, 2), p)                 # 65536 * 2 / 3 rounds to 43691; the pivot stays fixed
        assert want.a[0] == 43691 and want.t == [(65536 - 43691) * v for v in p]
        assert same_fields(host.xform_scale((3, 3, 3), (2, 2, 2), p), want)
    q = xm.quarter_turns(2, 1, (16, 16, 16))
    assert q.a == [0, 65536, 0, -65536, 0, 0, 0, 0, 65536] and q.t == [0, 65536 * 32, 0]


@pytest.mark.parametrize("axis,degrees,pivot", [((0, 0, 1), 30.0, (13.5, 17.25, 4.0)), ((0, 0, 2), 45.0, (5.0, 9.5, 0.0)),
                                                ((1, 2, -2), 30.0, (20.5, 3.0, 11.75)), ((1, 0, 0), -120.0, (0.0, 0.0, 0.0))])
def test_rotate_is_within_one_unit_of_the_rounded_closed_form(axis, degrees, pivot):
    got, want = host.xform_rotate(axis, degrees, pivot), xm.rotation(axis, degrees, pivot)
    assert np.abs(np.array(list(got.a)) - np.array(want.a)).max() <= 1
    assert np.abs(np.array(list(got.t)) - np.array(want.t)).max() <= 1
    assert got.material == -1 and list(got.dst_hi) == [2 ** 31 - 1] * 3
    if axis == (0, 0, 1):                                        # the closed form itself, by hand: 65536 cos 30, 65536 sin 30
        assert want.a == [56756, 32768, 0, -32768, 56756, 0, 0, 0, 65536]


def test_the_unit_compiled_for_the_cpu_runs_clean_under_the_sanitizers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostsim", "run.py"), "xform"], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout and "MISMATCH" not in r.stdout and "ERROR" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
