"""The voxel-list layer's kernels (csrc/tdt_voxlist.hip: last-of-run flags, (key, value) unique, gather, keys) at their launch
boundary, through the calls that reach them.  Blocks are 256 lanes and the flags kernels run n + 1 lanes, so a list of 255, 256
and 257 entries and a tree of exactly 256 voxels put n, n + 1 and the merge's nv + |B| on, just below and just above a block.
Everything is at depth 4, against the numpy list semantics of tests/test_gpu_region_edit.py and tests/morph_model.py, on a
single-device context and on a two-member one."""
import itertools

import numpy as np
import pytest

import morph_model as mm
from test_gpu_connect import bind_tree
from test_gpu_region_edit import apply_op, expected_bytes, inside
from tdt4230_project_raytracing_amd import rt

pytestmark = pytest.mark.gpu
DEPTH, N = 4, 16
CONTEXTS = [pytest.param(None, id="single"), pytest.param([0, 0], id="two-members")]


def tree_256():
    """256 voxels: a solid 6 x 6 x 6 block (so that two erosions leave something) and 40 scattered ones, materials 1..254."""
    rng = np.random.default_rng(256)
    blk = np.stack(np.meshgrid(*[np.arange(4, 10)] * 3, indexing="ij"), -1).reshape(-1, 3)
    rest = np.array([p for p in itertools.product(range(N), repeat=3) if not all(4 <= c <= 9 for c in p)])
    xyz = np.concatenate([blk, rest[rng.choice(len(rest), 40, replace=False)]])
    assert len(xyz) == 256 and len(np.unique(xyz, axis=0)) == 256
    return np.concatenate([xyz, rng.integers(1, 255, (256, 1))], 1).astype(np.int32)


def raw_list(n, V):
    """n entries in list order: voxels of V and fresh ones, 30 of them listed again later with another material (the later one
    must win), and one voxel off the grid (dropped); and B, what the list means."""
    rng = np.random.default_rng(n)
    free = np.array([p for p in itertools.product(range(N), repeat=3)])
    pts = free[rng.choice(len(free), n - 31, replace=False)]
    lst = np.concatenate([pts, rng.integers(1, 255, (len(pts), 1))], 1)
    if len(V):
        lst[:60, :3] = V[rng.choice(len(V), 60, replace=False), :3]          # (may repeat a fresh one: one more duplicate)
    dup = lst[5:35].copy()
    dup[:, 3] = (dup[:, 3] % 254) + 1                                       # another material, still 1..254
    raw = np.concatenate([lst[:100], [[N, 3, 3, 9]], lst[100:], dup]).astype(np.int32)
    assert len(raw) == n
    last = {}
    for v in raw:
        if (v[:3] >= 0).all() and (v[:3] < N).all():
            last[tuple(v[:3])] = v[3]
    assert len(last) < n - 1                                                # duplicates and the dropped key both decide
    return raw, np.array([[*k, m] for k, m in last.items()], np.int32)


@pytest.fixture(scope="module")
def tree():
    return tree_256()


@pytest.mark.parametrize("devices", CONTEXTS)
def test_voxel_list_edits_at_the_block_boundary(tree, devices):
    ctx = rt.Context(0, devices=devices)
    try:
        for base, n, op in itertools.product((np.zeros((0, 4), np.int32), tree), (255, 256, 257), (rt.REGION_SET, rt.REGION_FILL)):
            vbo, counter, V = bind_tree(ctx, base, DEPTH, room=700)
            assert np.array_equal(ctx.octree_extract().reshape(-1, 4), V) and len(V) == len(base)
            raw, B = raw_list(n, V)
            want_vox = apply_op(V, op, B, 0)
            want, n_want = expected_bytes(ctx, want_vox, DEPTH, vbo.read(np.uint32).nbytes)
            tag = (len(base), n, op)
            assert ctx.octree_edit_voxels(op, raw) == n_want, tag
            assert np.array_equal(vbo.read(np.uint32), want) and int(counter.read(np.uint32)[0]) == n_want, tag
            assert np.array_equal(ctx.octree_extract(), want_vox), tag
    finally:
        ctx.close()


@pytest.mark.parametrize("devices", CONTEXTS)
def test_extract_region_gathers_a_full_block(tree, devices):
    ctx = rt.Context(0, devices=devices)
    try:
        _, _, V = bind_tree(ctx, tree, DEPTH)
        for g in (rt.box((3, 0, 2), (11, 15, 9)), rt.box((0, 0, 0), (15, 15, 15)), rt.box((12, 12, 12), (12, 12, 12))):
            want = V[inside(V[:, :3], [g])]
            assert np.array_equal(ctx.octree_extract_region(g).reshape(-1, 4), want), (list(g.a), list(g.b))
        assert 0 < inside(V[:, :3], [rt.box((3, 0, 2), (11, 15, 9))]).sum() < 256
    finally:
        ctx.close()


@pytest.mark.parametrize("devices", CONTEXTS)
def test_morph_steps_on_a_full_block(tree, devices):
    ctx = rt.Context(0, devices=devices)
    try:
        _, _, V = bind_tree(ctx, tree, DEPTH)
        cache, sizes = {}, set()
        for op, radius, regions in itertools.product((rt.MORPH_DILATE, rt.MORPH_ERODE, rt.MORPH_SHELL), (1, 2), (None, [rt.box((0, 0, 0), (7, 15, 11))])):
            want = mm.morph(V, DEPTH, op, radius, 6, regions=regions, cache=cache)
            got = ctx.octree_extract_morph(op, radius, 6, regions=regions)
            assert got.shape == want.shape and np.array_equal(got, want), (op, radius, regions is not None)
            sizes.add(len(want))
        assert len(sizes) > 6 and 0 not in sizes                            # the cases differ, and none is empty
    finally:
        ctx.close()
