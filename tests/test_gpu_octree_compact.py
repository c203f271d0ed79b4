"""Voxel extraction and in-place compaction (tdt_octree_census / tdt_octree_extract / tdt_octree_compact): the GPU walk of the
logical tree must give what tests/octree_util.py's numpy walk gives, and compaction must rewrite the bound cells buffer into
exactly what the builder makes of those voxels — reclaiming the cells that place / remove edits leave behind, so that the
trace's LDS residency and the edit program's free pool come back."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_py
import tree_model
from octree_util import distinct_deltas, edit_setup, expand_cells, written_node
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def spread3(v):
    v = np.asarray(v, np.uint64)
    k = np.zeros_like(v)
    for b in range(10):
        k |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return k


def morton(vox):
    return (spread3(vox[:, 0]) << np.uint64(2)) | (spread3(vox[:, 1]) << np.uint64(1)) | spread3(vox[:, 2])


def sorted_expand(cells, depth):
    v = expand_cells(cells, depth)
    return np.ascontiguousarray(v[np.argsort(morton(v), kind="stable")])


def assert_extract_is_expand(got, cells, depth):
    """got == expand_cells(cells, depth) sorted by Morton key.  Past 2^21 voxels the comparison runs through a dense grid of
    materials instead of a CPU sort: equal counts, got strictly ascending, and every voxel of got found in the grid."""
    want = expand_cells(cells, depth)
    assert got.shape == want.shape
    if len(want) <= (1 << 21):
        assert np.array_equal(got, want[np.argsort(morton(want), kind="stable")])
        return
    kg = morton(got)
    assert (np.diff(kg.astype(np.int64)) > 0).all()
    grid = np.zeros(1 << (3 * depth), np.uint8)
    grid[morton(want)] = want[:, 3]
    del want
    assert (grid[kg] == got[:, 3]).all()


def census_np(cells_u32, depth):
    """The walk of tdt_octree_census in numpy: per level, the frontier of cells read (once per path)."""
    cells = np.asarray(cells_u32, np.uint32).reshape(-1, 8, 2)
    f = np.zeros(1, np.int64)
    reach = leaves = voxels = max_cell = 0
    for level in range(1, depth + 1):
        reach += f.size
        if f.size:
            max_cell = max(max_cell, int(f.max()))
        nodes = np.zeros((f.size, 8, 2), np.uint32)
        inb = f < len(cells)
        nodes[inb] = cells[f[inb]]
        t = nodes[..., 1]
        nl = int((t == 2).sum())
        leaves += nl
        voxels += nl << (3 * (depth - level))
        child = (t != 0) & (t != 2) if level < depth else np.zeros_like(t, bool)
        f = nodes[..., 0][child].astype(np.int64)
    return dict(reachable_cells=reach, leaf_nodes=leaves, voxels=voxels, max_cell=max_cell, buffer_cells=len(cells))


def bind_tree(ctx, cells, depth, counter=None):
    vbos = {0: rt.VertexBufferObject(ctx, np.ascontiguousarray(cells, np.uint32)),
            7: rt.VertexBufferObject(ctx, np.array([depth, 64, 1 << 10], np.int32))}
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, vbos[0])
    ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, vbos[7])
    if counter is not None:
        vbos["counter"] = rt.VertexBufferObject(ctx, np.array([counter], np.uint32))
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, vbos["counter"])
    return vbos


def monument_scene():
    z = np.load(os.path.join(GOLDEN, "monu1_ply_320x240_spp2_b6.npz"))
    return host.Scene({s: z[f"blob_{s}"] for s in (0, 1, 2, 3, 4, 6, 7)})


MODEL_LIMIT = 1 << 20                         # voxels up to which an expected tree is also checked against the numpy builder


def canonical(ctx, cells, depth, nbytes, model=True):
    """What compaction must leave in a buffer of nbytes: the builder's tree of the voxels, then zeros.  Up to MODEL_LIMIT voxels
    the GPU builder's bytes must also be those of the numpy builder (tests/tree_model.py), which shares no code with it;
    model=False: for a list the model does not take."""
    vox = sorted_expand(cells, depth)
    vbo, n = rt.octree_build_cells(ctx, vox, depth)
    built = vbo.read(np.uint32)
    if model and len(vox) <= MODEL_LIMIT:
        want = tree_model.build_cells(vox, depth)
        assert n == len(want) // 16 and built.size == want.size and np.array_equal(built, want), "the GPU builder differs from tree_model"
    out = np.zeros(nbytes // 4, np.uint32)
    out[: 16 * n] = built
    return out, n


def place_remove_deltas(rng, n, depth, cells, n_materials, free_only=False):
    """Up to n place edits (LEAF of a random material) in distinct cells of the edit walk's last level, and their removals;
    free_only: only where that cell holds no voxel yet (so that removing gives the tree back)."""
    d = distinct_deltas(rng, 4 * n if free_only else n, depth, cells)
    if free_only:
        d = d[[cells[2 * written_node(cells, p[:3], depth) + 1] == 0 for p in d]][:n]
    place = d.copy()
    place[:, 3] = 2.0
    place[:, 4] = rng.integers(0, n_materials, size=len(d))
    remove = d.copy()
    remove[:, 3] = 0.0
    remove[:, 4] = 0.0
    return place, remove


def run_edits(r, upd, dv, delta):
    dv.sub_data(0, np.ascontiguousarray(delta, np.float32))
    upd.dispatch_compute(len(delta), 1, 1)


# ---- 1. extraction and census ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["demo", "config1", "config2", "config3", "config5", "monument"])
def test_extract_and_census_equal_the_numpy_walk(name):
    scene = host.Scene.demo() if name == "demo" else monument_scene() if name == "monument" else host.Scene.config(int(name[-1]))
    depth = int(np.asarray(scene.blobs[7]).view(np.int32)[0])
    ctx = rt.Context(0)
    try:
        rt.upload_scene(ctx, scene)
        cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
        census = ctx.octree_census()
        assert census == {**census_np(cells, depth), "counter": -1}
        got = ctx.octree_extract()
        assert got.dtype == np.int32 and len(got) == census["voxels"]
        assert_extract_is_expand(got, cells, depth)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_extract_after_edit_sessions(oracle, mode):
    """Places and removes through the parallel (mode 0) and the ordered (mode 1) edit paths, then a collision-prone batch."""
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 4000, np.uint32)])
    rng = np.random.default_rng(11 + mode)
    place, remove = place_remove_deltas(rng, 300, depth, scene.blobs[0], 20)
    mixed = np.concatenate([place[:150], remove[:100]])
    r, upd, counter = edit_setup(scene, used, np.zeros(8 * 600, np.float32))
    try:
        r.ctx.edit_mode(mode)
        dv = rt.VertexBufferObject(r.ctx, np.zeros(8 * 600, np.float32))
        r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, dv)
        cells, c = np.ascontiguousarray(scene.blobs[0]).view(np.uint32), used
        for batch in (place, remove[:200], mixed):
            want, c = oracle_py.oracle_octree_update(oracle, host.Scene({**scene.blobs, 0: cells}), batch, c, (len(batch), 1, 1))
            run_edits(r, upd, dv, batch)
            cells = want
            got = r.ctx.octree_extract()
            assert np.array_equal(r.vbos[0].read(np.uint32), want)
            assert np.array_equal(got, sorted_expand(want, depth))
            census = r.ctx.octree_census()
            assert census == {**census_np(want, depth), "counter": c}
    finally:
        r.close()


def test_type_3_is_walked_as_a_parent():
    cells = np.zeros((3, 8, 2), np.uint32)
    cells[0, 5] = [1, 3]                       # treeLookup descends into any type that is neither EMPTY nor LEAF
    cells[0, 2] = [2, 1]
    cells[1, 0] = [4, 2]
    cells[1, 7] = [2, 7]                       # (on the last level: nothing)
    cells[2, 3] = [9, 2]
    ctx = rt.Context(0)
    try:
        bind_tree(ctx, cells.reshape(-1), 2, counter=3)
        got = ctx.octree_extract()
        assert got.tolist() == [[0, 3, 1, 10], [2, 0, 2, 5]]       # Morton order: key 19, then key 40
        assert ctx.octree_census() == dict(reachable_cells=3, leaf_nodes=2, voxels=2, max_cell=2, buffer_cells=3, counter=3)
    finally:
        ctx.close()


# ---- 2. canonical trees are left alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [1, 2, 3, 5])
def test_compact_is_idempotent_on_canonical_trees(cfg):
    scene = host.Scene.config(cfg)
    ctx = rt.Context(0)
    try:
        vbos = rt.upload_scene(ctx, scene)
        counter = rt.VertexBufferObject(ctx, np.array([12345], np.uint32))
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)
        before = vbos[0].read(np.uint32)
        n = ctx.octree_compact()
        assert n == scene.counts["cells"]
        assert np.array_equal(vbos[0].read(np.uint32), before)
        assert int(counter.read(np.uint32)[0]) == n
    finally:
        ctx.close()


# ---- 3. place then remove, then compact: the original bytes ----------------------------------------------------------
def test_undo_restores_the_original_bytes():
    """Config 2 rather than config 1: config 1's root has no EMPTY node, so its edits allocate only on the walk's last level,
    where the delta overwrites the fresh PARENT, and a place + remove leaves its bytes as they were."""
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    original = np.ascontiguousarray(scene.blobs[0]).view(np.uint32).copy()
    padded = np.concatenate([original, np.zeros(16 * 2000, np.uint32)])
    scene.blobs[0] = padded
    place, remove = place_remove_deltas(np.random.default_rng(3), 200, depth, padded, 20, free_only=True)
    assert len(place) >= 100
    r, upd, counter = edit_setup(scene, used, np.zeros(8 * 256, np.float32))
    try:
        dv = rt.VertexBufferObject(r.ctx, np.zeros(8 * 256, np.float32))
        r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, dv)
        run_edits(r, upd, dv, place)
        run_edits(r, upd, dv, remove)
        edited = r.vbos[0].read(np.uint32)
        assert int(counter.read(np.uint32)[0]) > used and not np.array_equal(edited, padded)
        n = r.compact()
        back = r.vbos[0].read(np.uint32)
        assert n == used and back.size == padded.size
        assert np.array_equal(back[: 16 * n], original) and not back[16 * n:].any()
        assert int(counter.read(np.uint32)[0]) == used
    finally:
        r.close()


# ---- 4. canonical form of random edited trees ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_compacted_bytes_are_the_builders_tree(seed):
    scene = host.Scene.config(2 if seed < 2 else 3)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 6000, np.uint32)])
    rng = np.random.default_rng(40 + seed)
    place, remove = place_remove_deltas(rng, 500, depth, scene.blobs[0], 20)
    r, upd, counter = edit_setup(scene, used, np.zeros(8 * 1000, np.float32))
    try:
        dv = rt.VertexBufferObject(r.ctx, np.zeros(8 * 1000, np.float32))
        r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, dv)
        run_edits(r, upd, dv, place)
        run_edits(r, upd, dv, remove[rng.permutation(len(remove))[: len(remove) // 2]])
        edited = r.vbos[0].read(np.uint32)
        before = r.ctx.octree_extract()
        want, n_want = canonical(r.ctx, edited, depth, edited.nbytes)
        n = r.compact()
        assert n == n_want
        assert np.array_equal(r.vbos[0].read(np.uint32), want)
        assert np.array_equal(r.ctx.octree_extract(), before)
        assert int(counter.read(np.uint32)[0]) == n
        gpu_built, _ = rt.octree_build_cells(r.ctx, before, depth)
        assert np.array_equal(gpu_built.read(np.uint32), want[: 16 * n])
    finally:
        r.close()


# ---- 5. residency comes back -----------------------------------------------------------------------------------------
def test_lds_residency_comes_back(oracle):
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 8000, np.uint32)])
    r, upd, counter = edit_setup(scene, used, np.zeros(8 * 4000, np.float32))
    try:
        r.render()
        assert r.ctx.last_variant()["resident"] == 1, "precondition: config 2 is LDS-resident"
        dv = rt.VertexBufferObject(r.ctx, np.zeros(8 * 4000, np.float32))
        r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, dv)
        rng = np.random.default_rng(5)
        for _ in range(8):
            cells = r.vbos[0].read(np.uint32)
            place, remove = place_remove_deltas(rng, 400, depth, cells, 20)
            run_edits(r, upd, dv, place)
            run_edits(r, upd, dv, remove)
            if int(counter.read(np.uint32)[0]) > 5120 + 64:
                break
        assert int(counter.read(np.uint32)[0]) > 5120
        r.render()
        assert r.ctx.last_variant()["resident"] == 0, "precondition: the dead cells pushed the tree out of the LDS table"
        r.compact()
        img = r.render()
        assert r.ctx.last_variant()["resident"] == 1
        compacted = host.Scene({**scene.blobs, 0: r.vbos[0].read(np.uint32)})
        assert (img.view(np.uint32) == oracle.render(compacted, r.camera, threads=4).view(np.uint32)).all()
    finally:
        r.close()


# ---- 6. capacity comes back ------------------------------------------------------------------------------------------
def _click(r, upd, dv, delta_row):
    d = np.zeros(8, np.float32)
    d[:5] = np.asarray(delta_row, np.float32)[:5]
    dv.sub_data(0, d)
    upd.dispatch_compute(1, 1, 1)


def _first_empty_level(cells, p, depth):
    """Level of the first EMPTY node the edit walk at p meets (None: a full walk); from there on it allocates a cell per level."""
    g = 1 << depth
    q = [int(c * g) for c in p]
    value = 0
    for level in range(1, depth):
        sh = depth - level
        i = (((2 * value + ((q[0] >> sh) & 1)) << 1) + ((q[1] >> sh) & 1) << 1) + ((q[2] >> sh) & 1)
        if cells[2 * i + 1] == 0:
            return level
        value = int(cells[2 * i])
    return None


def test_capacity_comes_back():
    scene = host.Scene.config(1)
    used, depth = scene.counts["cells"], scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32).copy()
    cells[8:16] = 0                                        # root octants 4..7 EMPTY (their subtrees are dead cells now)
    spare = 6
    scene.blobs[0] = np.concatenate([cells, np.zeros(16 * spare, np.uint32)])
    n_buf = used + spare
    g = 1 << (depth - 1)
    pos = [(np.array([x, y, z], np.float32) + np.float32(0.5)) / np.float32(g) for x in range(g) for y in range(g) for z in range(g)]
    # the probe allocates from the root down, so with the counter past the buffer its voxel lands outside; the others cycle the counter
    probe = [p for p in pos if (p >= 0.5).all() and _first_empty_level(cells, p, depth) == 1][0]
    cyclers = [p for p in pos if not (p >= 0.5).all() and _first_empty_level(cells, p, depth) is not None]
    r, upd, counter = edit_setup(scene, used, np.zeros(8, np.float32))
    try:
        dv = rt.VertexBufferObject(r.ctx, np.zeros(8, np.float32))
        r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, dv)
        for p in cyclers:                                  # place / remove until the counter passes the buffer
            _click(r, upd, dv, [*p, 2.0, 1.0])
            _click(r, upd, dv, [*p, 0.0, 0.0])
            if int(counter.read(np.uint32)[0]) > n_buf:
                break
        assert int(counter.read(np.uint32)[0]) > n_buf
        place = [*probe, 2.0, 2.0]
        n0 = len(r.ctx.octree_extract())
        _click(r, upd, dv, place)
        assert len(r.ctx.octree_extract()) == n0, "precondition: with the counter past the buffer, a place adds nothing"
        r.compact()
        assert len(r.ctx.octree_extract()) == n0
        _click(r, upd, dv, place)
        # the edit walk stops one level above max_depth: one placed voxel is a block of 2 x 2 x 2 finest-level voxels
        assert len(r.ctx.octree_extract()) == n0 + 8
    finally:
        r.close()


# ---- 7. ordering and errors ------------------------------------------------------------------------------------------
def test_edit_just_before_compact_is_included(oracle):
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 3000, np.uint32)])
    place, _ = place_remove_deltas(np.random.default_rng(21), 200, depth, scene.blobs[0], 20)
    want, _ = oracle_py.oracle_octree_update(oracle, scene, place, used, (len(place), 1, 1))
    r, upd, counter = edit_setup(scene, used, place)
    try:
        upd.dispatch_compute(len(place), 1, 1)             # no finish
        n = r.compact()
        expect, n_want = canonical(r.ctx, want, depth, want.nbytes)
        assert n == n_want and np.array_equal(r.vbos[0].read(np.uint32), expect)
    finally:
        r.close()


def test_errors():
    L = rt.lib()
    scene = host.Scene.config(1)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32).copy()
    ctx = rt.Context(0)
    try:
        out6 = (rt.ctypes.c_int64 * 6)()
        n = rt.ctypes.c_size_t(0)
        nc = rt.ctypes.c_uint32(0)
        for bound in ((), (0,), (7,)):
            for s in bound:
                v = rt.VertexBufferObject(ctx, cells if s == 0 else np.array([depth, 64, 128], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, v)
            assert L.tdt_octree_census(ctx.h, out6) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_extract(ctx.h, None, 0, rt.ctypes.byref(n)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_compact(ctx.h, rt.ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        vbos = bind_tree(ctx, cells, depth, counter=used_or(scene))
        # capacity too small: the count is reported, nothing is written
        total = len(expand_cells(cells, depth))
        buf = np.full((total, 4), -7, np.int32)
        assert L.tdt_octree_extract(ctx.h, buf.ctypes.data, total - 1, rt.ctypes.byref(n)) == rt.ERR_INVALID_VALUE
        assert n.value == total and (buf == -7).all()
        assert L.tdt_octree_extract(ctx.h, buf.ctypes.data, total, rt.ctypes.byref(n)) == rt.OK and n.value == total
        # a LEAF value of 254 extracts, but does not compact; the bytes stay as they were
        leaf = int(np.flatnonzero(cells[1::2] == 2)[0])
        bad = cells.copy()
        bad[2 * leaf] = 254
        vbos[0].sub_data(0, bad)
        assert ctx.octree_extract()[:, 3].max() == 255
        assert L.tdt_octree_compact(ctx.h, rt.ctypes.byref(nc)) == rt.ERR_INVALID_VALUE
        assert np.array_equal(vbos[0].read(np.uint32), bad) and int(vbos["counter"].read(np.uint32)[0]) == used_or(scene)
        bad[2 * leaf] = 0x7FFFFFFF
        vbos[0].sub_data(0, bad)
        assert L.tdt_octree_extract(ctx.h, None, 0, rt.ctypes.byref(n)) == rt.ERR_INVALID_VALUE
        # depth outside 1..10
        vbos[7].sub_data(0, np.array([11], np.int32))
        assert L.tdt_octree_census(ctx.h, out6) == rt.ERR_INVALID_VALUE
    finally:
        ctx.close()


def used_or(scene):
    return int(scene.counts["cells"])


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["single", "two-members"])
def test_a_misfit_leaves_n_cells_and_the_bytes_alone(devices):
    """Eight PARENT nodes that share one cell of eight different LEAFs: two cells whose canonical tree needs nine.  Compaction
    writes *n_cells only once the tree is installed, on a single-device context and on every replica alike."""
    cells = np.zeros((2, 8, 2), np.uint32)
    cells[0, :] = [1, 1]
    cells[1, :, 0], cells[1, :, 1] = np.arange(8), 2
    ctx = rt.Context(0, devices=devices)
    try:
        vbos = bind_tree(ctx, cells.reshape(-1), 2, counter=2)
        assert ctx.octree_census()["voxels"] == 64
        nc = rt.ctypes.c_uint32(777)
        assert rt.lib().tdt_octree_compact(ctx.h, rt.ctypes.byref(nc)) == rt.ERR_INVALID_VALUE
        assert "(9 cells) does not fit in the cells buffer (2 cells)" in rt.lib().tdt_last_error(ctx.h).decode()
        assert nc.value == 777
        assert np.array_equal(vbos[0].read(np.uint32), cells.reshape(-1)) and int(vbos["counter"].read(np.uint32)[0]) == 2
    finally:
        ctx.close()


def test_removing_every_voxel_compacts_to_one_cell():
    scene = host.Scene.config(1)
    used, depth = scene.counts["cells"], scene.max_depth
    vox = expand_cells(scene.blobs[0], depth)
    blocks = np.unique(vox[:, :3] >> 1, axis=0)             # every occupied cell of the edit walk's last level
    d = np.zeros((len(blocks), 8), np.float32)
    d[:, :3] = (blocks.astype(np.float32) + 0.5) / np.float32(1 << (depth - 1))
    r, upd, counter = edit_setup(scene, used, d)
    try:
        upd.dispatch_compute(len(d), 1, 1)
        assert len(r.ctx.octree_extract()) == 0
        assert r.compact() == 1
        assert not r.vbos[0].read(np.uint32).any()
        assert int(counter.read(np.uint32)[0]) == 1
        assert len(r.ctx.octree_extract()) == 0
        assert r.ctx.octree_census()["reachable_cells"] == 1
    finally:
        r.close()


# ---- 8. multi-device -------------------------------------------------------------------------------------------------
def test_multi_device_compaction_renders_like_a_single_device(oracle):
    scene = host.Scene.config(2)
    used, depth = scene.counts["cells"], scene.max_depth
    scene.blobs[0] = np.concatenate([scene.blobs[0], np.zeros(16 * 3000, np.uint32)])
    place, remove = place_remove_deltas(np.random.default_rng(17), 300, depth, scene.blobs[0], 20)
    cam = host.camera_reference_pose(96, 64, 2, 3)
    outs = []
    for devices in (None, [0, 0]):
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            upd = rt.ComputeShader(r.ctx, rt.PROGRAM_OCTREE_UPDATE)
            counter = rt.VertexBufferObject(r.ctx, np.array([used], np.uint32))
            r.ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)
            dv = rt.VertexBufferObject(r.ctx, np.zeros(8 * 300, np.float32))
            r.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, dv)
            run_edits(r, upd, dv, place)
            run_edits(r, upd, dv, remove[::2])
            r.render()
            n = r.compact()
            outs.append((n, r.vbos[0].read(np.uint32), int(counter.read(np.uint32)[0]), r.render(), r.ctx.octree_extract()))
        finally:
            r.close()
    (n1, c1, k1, img1, v1), (n2, c2, k2, img2, v2) = outs
    assert n1 == n2 == k1 == k2 and np.array_equal(c1, c2) and np.array_equal(v1, v2)
    assert (img1.view(np.uint32) == img2.view(np.uint32)).all()
    assert (img1.view(np.uint32) == oracle.render(host.Scene({**scene.blobs, 0: c1}), cam, threads=4).view(np.uint32)).all()


# ---- 9. the demo -----------------------------------------------------------------------------------------------------
def test_demo_click_and_compact_equals_the_oracle(oracle, tmp_path):
    exe = build.build_demo()
    out = str(tmp_path / "frame.pfm")
    w, h = 128, 96
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cam = host.camera_reference_pose(w, h, 2, 6)
    r = rt.Renderer(scene, cam)
    try:
        xy = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.int32)
        picks = r.pick(xy)
    finally:
        r.close()
    order = np.argsort(np.abs(xy[:, 0] - w // 2) + np.abs(xy[:, 1] - h // 2), kind="stable")
    px = delta = None
    for i in order:
        if picks[i]["status"] == rt.RAY_HIT and picks[i]["fresh_record"]:
            try:
                delta = host.pick_edit_delta(picks[i], scene, 1, 3.0)
            except ValueError:
                continue
            px = xy[i]
            break
    assert px is not None
    p = subprocess.run([exe, "--config", "2", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "6", "--pick", f"{px[0]},{px[1]}",
                        "--click", "left", "--material", "3", "--compact", "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert re.search(r"edit place", p.stdout), p.stdout
    edited, _ = oracle_py.oracle_octree_update(oracle, scene, delta[:5], scene.counts["cells"], (0, 1, 0))
    want, n = canonical_host(edited, depth)
    census = {m.group(1): [int(x) for x in m.groups()[1:]] for m in re.finditer(
        r"census (\w+) reachable (\d+) leaves (\d+) voxels (\d+) max_cell (\d+) buffer_cells (\d+) counter (-?\d+)", p.stdout)}
    assert set(census) == {"before", "after"}
    assert census["before"][:4] == [census_np(edited, depth)[k] for k in ("reachable_cells", "leaf_nodes", "voxels", "max_cell")]
    assert census["after"][0] == n and census["after"][5] == n and census["after"][2] == census["before"][2]
    assert f"compact cells {n}" in p.stdout
    ref = oracle.render(host.Scene({**scene.blobs, 0: want}), cam, threads=8)
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF4"
        fw, fh = map(int, f.readline().split())
        f.readline()
        img = np.frombuffer(f.read(), "<f4").reshape(fh, fw, 4)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


def canonical_host(cells, depth):
    ctx = rt.Context(0)
    try:
        return canonical(ctx, cells, depth, np.asarray(cells).nbytes)
    finally:
        ctx.close()
