"""Exact Euclidean distance on the GPU (tdt_octree_morph_round / tdt_octree_extract_morph_round / tdt_octree_distance_field): the
voxel lists and the field must equal the numpy model (tests/distance_model.py) element for element, nearest voxels and inherited
materials included, and the edit form must leave in the bound cells buffer exactly what tdt_octree_edit_voxels of the model's
list leaves.  Every comparison is exact equality."""
import ctypes
import itertools
import re
import subprocess

import numpy as np
import pytest

import distance_model as dm
import morph_model as mm
from test_gpu_connect import bind_tree, block
from test_gpu_fill import strided_bbox_tree
from test_gpu_region_edit import bind_cells, built_cells, padded, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
OPS = (rt.MORPH_DILATE, rt.MORPH_ERODE, rt.MORPH_OPEN, rt.MORPH_CLOSE, rt.MORPH_SHELL)
GROWS = (rt.MORPH_DILATE, rt.MORPH_CLOSE)
EDGES = (0, 1, 31, 32, 33, 62, 63, 64, 65, 126, 127)


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def same(got, want, tag=""):
    assert got.shape == want.shape and np.array_equal(got, want), tag


def delta_of(V, want):
    """(region op, list) that turns V into want: the new voxels to FILL, or the removed ones to CLEAR."""
    kv, kw = mm._keys(V[:, :3]), mm._keys(want[:, :3])
    new, gone = want[~np.isin(kw, kv)], V[~np.isin(kv, kw)]
    assert not (len(new) and len(gone))
    return (rt.REGION_FILL, new) if len(new) or not len(gone) else (rt.REGION_CLEAR, gone)


def check_edit(ctx, V, depth, want, tag, **kw):
    """octree_morph_round on a fresh tree of V: the bytes tdt_octree_edit_voxels of the model's list leaves, which are the
    builder's tree of the model's result."""
    built = built_cells(ctx, want, depth, model=len(want) <= 1 << 16)
    have = len(built_cells(ctx, V, depth, model=False)) // 16
    room = max(len(built) // 16 - have, 0) + 8
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    n = ctx.octree_morph_round(**kw)
    got = vbo.read(np.uint32)
    assert n == len(built) // 16 and int(counter.read(np.uint32)[0]) == n, tag
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    assert ctx.octree_edit_voxels(*delta_of(V, want)) == n, tag
    assert np.array_equal(got, vbo.read(np.uint32)) and np.array_equal(got, padded(built, got.nbytes)), tag


# ---- 1. random trees -----------------------------------------------------------------------------------------------------------
def random_tree(depth):
    """Solid balls of several materials, salt and pepper: every op changes it, at every radius of the suite."""
    rng = np.random.default_rng(77 + depth)
    n = 1 << depth
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1)
    solid = np.zeros((n, n, n), bool)
    for _ in range(3):
        c, r = rng.integers(0, n, 3), rng.integers(n // 4, n // 2)
        solid |= ((g - c) ** 2).sum(-1) <= r * r
    solid ^= rng.random((n, n, n)) < 0.04
    p = np.argwhere(solid)
    return sort_vox(np.concatenate([p, 1 + (p[:, :1] // 2 + p[:, 1:2] + 3 * p[:, 2:3]) % 254], 1))


def axis_ties(V, depth):
    """Empty voxels with an occupied voxel at distance 1 on both sides along x: two nearest voxels, a tie for sure."""
    occ = dm.grid_of(V, depth) > 0
    return int((~occ[1:-1] & occ[:-2] & occ[2:]).sum())


@pytest.mark.parametrize("radius2", [1, 2, 3, 5, 9, 16])
@pytest.mark.parametrize("depth", [3, 4, 5, 6])
def test_random_trees_equal_the_model(ctx, depth, radius2):
    n = 1 << depth
    V = random_tree(depth)
    assert 0 < len(V) < n ** 3 and axis_ties(V, depth) > 0
    mask = [rt.box((1, 0, 2), (n // 2, n - 2, n - 1)), rt.sphere((n // 2, n // 2, n // 3), n // 3)]
    bind_tree(ctx, V, depth)
    cases = []
    for op in OPS:
        borders = (0, 1) if op in (rt.MORPH_ERODE, rt.MORPH_SHELL) else (0,)
        materials = (None, 17) if op in GROWS else (None,)
        cases += [dict(op=op, radius2=radius2, border=b, material=m) for b in borders for m in materials]
    cases += [dict(op=op, radius2=radius2, regions=mask, material=m, border=radius2 % 2) for op, m in zip(OPS, (None, 250, None, None, None))]
    changed = set()
    for kw in cases:
        want = dm.round_op(V, depth, **kw)
        same(ctx.octree_extract_morph_round(**kw), want, kw)
        if not np.array_equal(want, V):
            changed.add(kw["op"])
    # every op changes the tree, by the model alone (once the erosion is empty, at the larger radii, the shell is V itself)
    assert changed >= set(OPS) - {rt.MORPH_SHELL} and (rt.MORPH_SHELL in changed or radius2 > 3)
    same(ctx.octree_extract_morph_round(rt.MORPH_DILATE, radius2, regions=[]), V, "an empty mask")
    same(ctx.octree_extract(), V, "the tree is untouched")
    for kw in cases:                                            # the edit form of every case
        check_edit(ctx, V, depth, dm.round_op(V, depth, **kw), kw, **kw)
    vbo, counter, _ = bind_tree(ctx, V, depth)
    before = vbo.read(np.uint32)
    ctx.octree_morph_round(rt.MORPH_ERODE, radius2, regions=[])   # an empty mask installs the canonical tree of V itself
    assert np.array_equal(vbo.read(np.uint32), before)


# ---- 2. word, tile and halo boundaries -----------------------------------------------------------------------------------------
def boundary_voxels(depth, axis):
    """One voxel at every coordinate of EDGES along `axis` (neighbouring coordinates make pairs), each of another material,
    staggered on the two other axes."""
    n = 1 << depth
    out = []
    for k, c in enumerate(e for e in EDGES if e < n):
        p = [0, 0, 0]
        p[axis] = c
        p[(axis + 1) % 3] = (5 + 23 * k) % n
        p[(axis + 2) % 3] = (n - 3 - 37 * k) % n
        out.append([*p, 10 + k])
    return sort_vox(np.array(out, np.int32))


@pytest.mark.parametrize("radius2", [1, 1024, 1600, 4096])
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("depth", [6, 7])
def test_word_tile_and_halo_boundaries(ctx, depth, axis, radius2):
    n = 1 << depth
    V = boundary_voxels(depth, axis)
    assert len(V) <= dm.SPARSE                                  # the all-pairs form of the model is the yardstick
    assert dm.sparse_ties(V, depth) > 0                         # tied nearest voxels exist: inherited materials depend on the rule
    want = dm.round_op(V, depth, rt.MORPH_DILATE, radius2)
    assert len(set(want[:, 3])) == len(V)
    bind_tree(ctx, V, depth)
    same(ctx.octree_extract_morph_round(rt.MORPH_DILATE, radius2), want, "dilate, inherited")
    lo, hi = [0, 0, 0], [n - 1, n - 1, n - 1]
    lo[(axis + 1) % 3], hi[(axis + 1) % 3] = 3, min(n - 2, 40)  # a slab, unaligned
    f, near = ctx.octree_distance_field(lo, hi, radius2, nearest=True)
    wf, wn = dm.field(V, depth, lo, hi, radius2)
    same(f, wf, "field")
    same(near, wn, "nearest")


TIE_BASES = {6: ((31, 20, 9), (59, 33, 31), (3, 59, 40)), 7: ((63, 20, 9), (123, 65, 31), (3, 123, 96))}


def tie_pairs(depth):
    """Pairs placed so that a tie plane, an axis tie and a diagonal tie are each hit, on every axis; around word boundaries."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for base in TIE_BASES[depth]:
            q = np.array([base[(k - a) % 3] for k in range(3)])
            e = np.eye(3, dtype=int)
            out.append([q - e[a], q + e[a]])                                        # q itself ties along the axis
            out.append([q - 3 * e[a] + 2 * e[b], q + 3 * e[a] + 2 * e[b]])          # an even separation: a whole tie plane
            out.append([q + e[a] + 2 * e[b], q + 2 * e[a] + e[b]])                  # (1, 2, 0) against (2, 1, 0)
            out.append([q - e[b] - 2 * e[c], q - 2 * e[b] - e[c]])
    return out


@pytest.mark.parametrize("case", range(len(tie_pairs(6))))
@pytest.mark.parametrize("depth", [6, 7])
def test_tied_pairs_follow_the_order(ctx, depth, case):
    n = 1 << depth
    pair = np.array(tie_pairs(depth)[case])
    assert pair.min() >= 0 and pair.max() < n
    V = sort_vox(np.concatenate([pair, [[5], [200]]], 1))
    assert len(np.unique(V[:, :3], axis=0)) == 2 and dm.sparse_ties(V, depth) > 0
    bind_tree(ctx, V, depth)
    for radius2 in (5, 9, 1024):
        want = dm.round_op(V, depth, rt.MORPH_DILATE, radius2)
        assert set(want[:, 3]) == {5, 200}
        same(ctx.octree_extract_morph_round(rt.MORPH_DILATE, radius2), want, radius2)
    f, near = ctx.octree_distance_field((0, 0, 0), (n - 1, n - 1, n - 1), 4096, nearest=True)
    wf, wn = dm.field(V, depth, (0, 0, 0), (n - 1, n - 1, n - 1), 4096)
    same(f, wf)
    same(near, wn)


# ---- 3. grid faces -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 4, 5])
def test_grid_faces(ctx, depth):
    n = 1 << depth
    full = block((0, 0, 0), (n - 1, n - 1, n - 1), 3)
    corner = block((0, 0, n // 2), (n // 2, n - 1, n - 1), 9)    # touches the faces x = 0, y = 0 and n - 1, z = n - 1
    for V in (sort_vox(full), sort_vox(corner)):
        bind_tree(ctx, V, depth)
        for radius2, border, op in itertools.product((1, 3, 4, 4096), (0, 1), (rt.MORPH_ERODE, rt.MORPH_SHELL, rt.MORPH_DILATE, rt.MORPH_OPEN, rt.MORPH_CLOSE)):
            want = dm.round_op(V, depth, op, radius2, border=border)
            same(ctx.octree_extract_morph_round(op, radius2, border=border), want, (len(V), radius2, border, op))
        for radius2, border in ((1, 0), (4, 1), (4096, 0)):
            check_edit(ctx, V, depth, dm.round_op(V, depth, rt.MORPH_ERODE, radius2, border=border), (radius2, border), op=rt.MORPH_ERODE,
                       radius2=radius2, border=border)
    want = dm.round_op(sort_vox(full), depth, rt.MORPH_ERODE, 1, border=0)
    assert len(want) == max(n - 2, 0) ** 3                       # the outside is empty: one layer goes
    assert len(dm.round_op(sort_vox(full), depth, rt.MORPH_ERODE, 4096, border=1)) == n ** 3
    check_edit(ctx, sort_vox(corner), depth, dm.round_op(sort_vox(corner), depth, rt.MORPH_DILATE, 5), "dilate clipped", op=rt.MORPH_DILATE, radius2=5)


# ---- 4. against the step-wise unit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [4, 6])
def test_against_the_stepwise_morphology(ctx, depth):
    V = random_tree(depth)
    built = built_cells(ctx, mm.morph(V, depth, mm.DILATE, 2, 6), depth)
    room = len(built) // 16 + 8
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    ctx.octree_morph_round(rt.MORPH_DILATE, 1)
    ctx.octree_morph_round(rt.MORPH_DILATE, 1)
    twice = vbo.read(np.uint32)
    vbo, counter, _ = bind_tree(ctx, V, depth, room)
    ctx.octree_morph(rt.MORPH_DILATE, 2, 6)
    assert np.array_equal(twice, vbo.read(np.uint32))           # inherited materials included: the tie rule is the first offset's
    same(ctx.octree_extract_morph_round(rt.MORPH_DILATE, 3, material=40), ctx.octree_extract_morph(rt.MORPH_DILATE, 1, 26, material=40))
    same(ctx.octree_extract_morph_round(rt.MORPH_ERODE, 3, border=1), ctx.octree_extract_morph(rt.MORPH_ERODE, 1, 26, border=1))


# ---- 5. the field --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_d2", [1, 9, 4096])
def test_distance_field(ctx, max_d2):
    depth, n = 5, 32
    V = random_tree(depth)
    vbo, counter, _ = bind_tree(ctx, V, depth)
    before = vbo.read(np.uint32)
    occ = dm.grid_of(V, depth) > 0
    for lo, hi in (((0, 0, 0), (n - 1, n - 1, n - 1)), ((3, 5, 1), (29, 17, 30)), ((7, 0, 0), (7, n - 1, n - 1)), ((0, 13, 2), (n - 1, 13, 2)),
                   ((30, 31, 0), (30, 31, 0))):
        for border in (0, 1):
            wf, wn = dm.field(V, depth, lo, hi, max_d2, border)
            same(ctx.octree_distance_field(lo, hi, max_d2, border), wf, (lo, hi, border))
            f, near = ctx.octree_distance_field(lo, hi, max_d2, border, nearest=True)
            same(f, wf)
            same(near, wn)
            o = occ[tuple(slice(lo[a], hi[a] + 1) for a in range(3))].transpose(2, 1, 0)
            assert ((f < 0) == o).all() and (np.abs(f) >= 1).all() and (np.abs(f) <= max_d2 + 1).all()      # sign and clamp
            none = (near == -1).all(-1)
            assert (none == (~o & (f == max_d2 + 1))).all()                                              # the {-1, -1, -1} rule
    assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345
    # the count-only call and the short capacity
    L = rt.lib()
    lo, hi = (ctypes.c_int32 * 3)(1, 2, 3), (ctypes.c_int32 * 3)(4, 4, 4)
    nv = ctypes.c_size_t(0)
    assert L.tdt_octree_distance_field(ctx.h, lo, hi, max_d2, 0, None, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == 4 * 3 * 2
    out = np.full(24, 777, np.int32)
    nv = ctypes.c_size_t(0)
    assert L.tdt_octree_distance_field(ctx.h, lo, hi, max_d2, 0, out.ctypes.data, None, 23, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
    assert nv.value == 24 and (out == 777).all()


def test_empty_tree(ctx):
    depth = 4
    vbo, counter, _ = bind_tree(ctx, np.zeros((0, 4), np.int32), depth, 4)
    f, near = ctx.octree_distance_field((0, 0, 0), (15, 15, 15), 9, nearest=True)
    assert (f == 10).all() and (near == -1).all()
    for op in OPS:
        assert len(ctx.octree_extract_morph_round(op, 4)) == 0
        assert ctx.octree_morph_round(op, 4) == 1
        assert not vbo.read(np.uint32).any() and int(counter.read(np.uint32)[0]) == 1


# ---- 6. errors and limits ------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(ctx):
    L = rt.lib()
    depth = 5
    V = random_tree(depth)
    nc, nv = ctypes.c_uint32(0), ctypes.c_size_t(0)
    ok = rt.Round(rt.MORPH_ERODE, 1, -1, 0)
    lo3, hi3 = (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(3, 3, 3)
    fresh = rt.Context(0)
    try:
        for bound in ((), (0,), (7,)):
            for s in bound:
                v = rt.VertexBufferObject(fresh, np.zeros(16, np.uint32) if s == 0 else np.array([depth, 64, 32], np.int32))
                fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, v)
            assert L.tdt_octree_morph_round(fresh.h, ctypes.byref(ok), None, 0, ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract_morph_round(fresh.h, ctypes.byref(ok), None, 0, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_distance_field(fresh.h, lo3, hi3, 4, 0, None, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            fresh.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
    finally:
        fresh.close()
    vbo, counter, _ = bind_tree(ctx, V, depth, 16)
    cells = vbo.read(np.uint32)

    def unchanged():
        return np.array_equal(vbo.read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 12345

    bad_shape = rt.box((0, 0, 0), (1, 1, 1))
    bad_shape.shape = 7
    M, X, F = ctx.octree_morph_round, ctx.octree_extract_morph_round, ctx.octree_distance_field
    cases = [lambda: M(5, 1), lambda: M(-1, 1), lambda: M(rt.MORPH_ERODE, 0), lambda: M(rt.MORPH_ERODE, 4097), lambda: M(rt.MORPH_ERODE, -4),
             lambda: M(rt.MORPH_DILATE, 1, material=254), lambda: M(rt.MORPH_DILATE, 1, material=-2), lambda: M(rt.MORPH_ERODE, 1, border=2),
             lambda: M(rt.MORPH_ERODE, 1, border=-1), lambda: M(rt.MORPH_ERODE, 1, regions=bad_shape),
             lambda: M(rt.MORPH_ERODE, 1, regions=rt.sphere((1, 1, 1), -1)),
             lambda: X(7, 1), lambda: X(rt.MORPH_SHELL, 0), lambda: X(rt.MORPH_SHELL, 5000), lambda: X(rt.MORPH_CLOSE, 1, material=300),
             lambda: X(rt.MORPH_SHELL, 1, border=3), lambda: X(rt.MORPH_SHELL, 1, regions=bad_shape),
             lambda: F((0, 0, 0), (3, 3, 3), 0), lambda: F((0, 0, 0), (3, 3, 3), 4097), lambda: F((0, 0, 0), (3, 3, 3), 4, border=2),
             lambda: F((-1, 0, 0), (3, 3, 3), 4), lambda: F((0, 0, 0), (3, 32, 3), 4), lambda: F((0, 4, 0), (3, 3, 3), 4)]
    for i, f in enumerate(cases):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE and unchanged(), i
    for rc in (L.tdt_octree_morph_round(ctx.h, None, None, 0, ctypes.byref(nc)),
               L.tdt_octree_morph_round(ctx.h, ctypes.byref(ok), None, 1, ctypes.byref(nc)),
               L.tdt_octree_extract_morph_round(ctx.h, ctypes.byref(ok), None, 2, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_morph_round(ctx.h, None, None, 0, None, 0, ctypes.byref(nv)),
               L.tdt_octree_extract_morph_round(ctx.h, ctypes.byref(ok), None, 0, None, 0, None),
               L.tdt_octree_distance_field(ctx.h, None, hi3, 4, 0, None, None, 0, ctypes.byref(nv)),
               L.tdt_octree_distance_field(ctx.h, lo3, None, 4, 0, None, None, 0, ctypes.byref(nv)),
               L.tdt_octree_distance_field(ctx.h, lo3, hi3, 4, 0, None, None, 0, None)):
        assert rc == rt.ERR_INVALID_VALUE and unchanged()
    # the extract form's short capacity: the count, nothing written
    want = dm.round_op(V, depth, rt.MORPH_SHELL, 2)
    out = np.zeros((len(want), 4), np.int32)
    shell = rt.Round(rt.MORPH_SHELL, 2, -1, 0)
    assert L.tdt_octree_extract_morph_round(ctx.h, ctypes.byref(shell), None, 0, out.ctypes.data, len(want) - 1, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
    assert nv.value == len(want) and not out.any()
    # a LEAF value >= 254 cannot be rebuilt: every form refuses it
    bad = cells.copy()
    leaf = np.flatnonzero((bad[1::2] == 2) & (bad[0::2] < 254))[0]
    bad[2 * int(leaf)] = 254
    vbo2, counter2 = bind_cells(ctx, bad, len(bad) // 16)
    for f in (lambda: M(rt.MORPH_ERODE, 1), lambda: X(rt.MORPH_ERODE, 1), lambda: F((0, 0, 0), (3, 3, 3), 4)):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE
        assert np.array_equal(vbo2.read(np.uint32), bad) and int(counter2.read(np.uint32)[0]) == 12345
    # a DILATE that does not fit: the cell count it needs, nothing written; the same call on a buffer of that size succeeds
    vbo3, counter3, V1 = bind_tree(ctx, np.array([[32, 32, 32, 5]], np.int32), 6)
    chain = vbo3.read(np.uint32)
    built = built_cells(ctx, dm.round_op(V1, 6, rt.MORPH_DILATE, 4), 6)
    need = len(built) // 16
    assert need > len(chain) // 16
    with pytest.raises(rt.TdtError) as e:
        M(rt.MORPH_DILATE, 4)
    assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
    assert np.array_equal(vbo3.read(np.uint32), chain) and int(counter3.read(np.uint32)[0]) == 12345
    vbo3, counter3 = bind_cells(ctx, chain, need)
    assert M(rt.MORPH_DILATE, 4) == need
    assert np.array_equal(vbo3.read(np.uint32), built) and int(counter3.read(np.uint32)[0]) == need


def test_domain_cap(ctx):
    """Two voxels at opposite corners: at depth 10 the domain is the whole grid, 2^30 voxels, and is refused before any volume is
    allocated; at depth 8 it is 2^24 and runs."""
    for depth in (10, 8):
        n = 1 << depth
        V = sort_vox(np.array([[0, 0, 0, 3], [n - 1, n - 1, n - 1, 8]], np.int32))
        vbo, counter, _ = bind_tree(ctx, V, depth, 64)
        cells = vbo.read(np.uint32)
        if depth == 10:
            for f in (lambda: ctx.octree_morph_round(rt.MORPH_DILATE, 1), lambda: ctx.octree_extract_morph_round(rt.MORPH_SHELL, 4)):
                with pytest.raises(rt.TdtError) as e:
                    f()
                assert e.value.code == rt.ERR_INVALID_VALUE and "domain" in str(e.value)
                assert np.array_equal(vbo.read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 12345
            with pytest.raises(rt.TdtError) as e:                # a field box above 2^26 voxels (a box within that limit cannot outgrow the domain cap)
                ctx.octree_distance_field((0, 0, 0), (n - 1, n - 1, 64), 1)
            assert e.value.code == rt.ERR_INVALID_VALUE
        else:
            got = ctx.octree_extract_morph_round(rt.MORPH_DILATE, 4, material=None)
            ball = np.array([(x, y, z) for x in range(3) for y in range(3) for z in range(3) if x * x + y * y + z * z <= 4])
            want = sort_vox(np.concatenate([np.concatenate([ball, np.full((len(ball), 1), 3)], 1),
                                            np.concatenate([n - 1 - ball, np.full((len(ball), 1), 8)], 1)]))
            same(got, want)
            check_edit(ctx, V, depth, want, "depth 8", op=rt.MORPH_DILATE, radius2=4)


def test_two_share_multi_device_edit_reaches_both_replicas():
    """A two-share context shards the frame over its members, so the frame after the edit shows every replica's cells: it must be,
    bit for bit, the single-device frame after the same edit and the frame of a fresh upload of the model's tree."""
    scene = host.Scene.config(2)
    depth = scene.max_depth
    full = sum(8 ** l for l in range(depth))                   # no tree of this depth has more cells: any result fits
    scene.blobs[0] = padded(np.ascontiguousarray(scene.blobs[0]).view(np.uint32).ravel(), 64 * full)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            V = r.ctx.octree_extract()
            c = V[len(V) // 2, :3].astype(int)
            mask = [rt.sphere(c, 12)]
            preview = r.ctx.octree_extract_morph_round(rt.MORPH_CLOSE, 5)
            n = r.ctx.octree_morph_round(rt.MORPH_CLOSE, 5)
            n2 = r.ctx.octree_morph_round(rt.MORPH_SHELL, 4, regions=mask)
            field = r.ctx.octree_distance_field((0, 0, 0), (63, 63, 63), 9)
            outs.append((n, n2, r.vbos[0].read(np.uint32), r.render(), r.ctx.octree_extract(), preview, field))
            if devices:
                assert rt.lib().tdt_ctx_device_count(r.ctx.h) == 2
        finally:
            r.close()
    one, two = outs
    for k, (a, b) in enumerate(zip(one, two)):                  # counts, cells, frame (by its bits), tree, preview, field
        if isinstance(a, np.ndarray) and a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), k
    closed = dm.round_op(V, depth, rt.MORPH_CLOSE, 5)
    same(two[5], closed, "preview")
    want = dm.round_op(closed, depth, rt.MORPH_SHELL, 4, regions=mask)
    same(two[4], want, "the tree after both edits")
    same(two[6], dm.field(want, depth, (0, 0, 0), (63, 63, 63), 9)[0], "field")
    ctx = rt.Context(0)
    try:
        built = built_cells(ctx, want, depth, model=False)
    finally:
        ctx.close()
    assert two[1] == len(built) // 16 and np.array_equal(two[2], padded(built, 64 * full))
    fresh = rt.Renderer(host.Scene({**scene.blobs, 0: padded(built, 64 * full)}), cam)
    try:
        ref = fresh.render()
    finally:
        fresh.close()
    assert (two[3].view(np.uint32) == ref.view(np.uint32)).all()


# ---- 7. the demo ---------------------------------------------------------------------------------------------------------------
def test_demo_morph_round_leaves_the_model_tree(tmp_path):
    exe = build.build_demo()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    room = len(np.asarray(scene.blobs[0]).view(np.uint32)) // 16
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        V = ctx.octree_extract()
        want = dm.round_op(V, depth, rt.MORPH_DILATE, 5, material=9, border=1)
        n = len(built_cells(ctx, want, depth)) // 16
        del vbos
    finally:
        ctx.close()
    assert len(want) > len(V)
    p = subprocess.run([exe, "--config", "2", "--size", "64x48", "--spp", "1", "--bounce", "2", "--cells", str(max(room, n)), "--morph-round",
                        "dilate:5", "--material", "9", "--border", "1", "--out", str(tmp_path / "frame.pfm")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(rf"morph-round dilate:5 border 1 cells {n}\b", p.stdout), p.stdout


# ---- 8. a list longer than one trip of the bounding box's strided loop ---------------------------------------------------------
def test_list_longer_than_the_bounding_box_launch(ctx):
    """The tree of test_gpu_fill.py whose bounding box is owed to the later trips of tdt_bitvol.hip's strided loop: a round op
    sizes its domain by that box, the field rasterises the same long list into a box of its own."""
    depth, V, _ = strided_bbox_tree()
    bind_tree(ctx, V, depth)
    for material in (None, 9):
        want = dm.round_op(V, depth, rt.MORPH_DILATE, 1, material)
        assert len(want) > len(V) and set(want[:, 3]) == ({int(V[0, 3])} if material is None else {int(V[0, 3]), material + 1})
        same(ctx.octree_extract_morph_round(rt.MORPH_DILATE, 1, material), want, material)
    lo, hi = (5, 6, 7), (14, 12, 13)                            # across the shell's corner: outside, wall and cavity
    f, near = ctx.octree_distance_field(lo, hi, 9, nearest=True)
    wf, wn = dm.field(V, depth, lo, hi, 9)
    assert (wf < 0).any() and (wf > 0).any()
    same(f, wf, "field")
    same(near, wn, "nearest")
