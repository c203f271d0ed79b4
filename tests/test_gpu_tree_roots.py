"""The two roots every edit suite rests on, against numpy models that share no code with them: the GPU builder
(tdt_octree_build_cells, csrc/tdt_build.hip) must write the bytes of tests/tree_model.py's build_cells, depth 10 included,
and the GPU walk (tdt_octree_census / tdt_octree_extract / tdt_octree_compact, csrc/tdt_compact.hip) must give what
octree_util.expand_cells and census_np give on trees the GPU builder never saw: the model's own cells, hand-made trees whose
shared cells force both of the walk's retries, and trees whose numbering is not breadth-first.  The inputs and their
preconditions are tests/tree_cases.py, proved on the CPU by tests/test_tree_cases.py.  Every comparison is bit for bit."""
import functools

import numpy as np
import pytest

import tree_cases as tc
import tree_model
from octree_util import expand_cells
from test_gpu_octree_compact import bind_tree, census_np
from tdt4230_project_raytracing_amd import rt

pytestmark = pytest.mark.gpu
FAMILIES = {name: (depth, vox) for name, depth, vox in tc.families()}
SMALL = [n for n in FAMILIES if tc.is_small(n)]


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def model(name):
    depth, vox = FAMILIES[name]
    m = tree_model.build_cells(vox, depth)
    m.setflags(write=False)
    return m


def bind(ctx, cells, depth, counter=None):
    """bind_tree, and no counter left bound from an earlier test when none is asked for."""
    if counter is None:
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, None)
    return bind_tree(ctx, cells, depth, counter=counter)


def census_of(cells, depth, counter=-1):
    return {**census_np(cells, depth), "counter": counter}


def assert_built_is_model(ctx, vox, depth, want):
    vbo, n = rt.octree_build_cells(ctx, vox, depth)
    assert n == len(want) // 16
    got = vbo.read(np.uint32)
    assert got.size == want.size and np.array_equal(got, want)


def assert_walk_is_numpy(ctx, cells, depth, want_vox):
    """census and extract of the bound `cells` against the numpy walks (want_vox: the voxels in Morton order)."""
    assert ctx.octree_census() == census_of(cells, depth)
    got = ctx.octree_extract()
    assert got.dtype == np.int32 and got.shape == want_vox.shape and np.array_equal(got, want_vox)


# ---- a. the builder against the model --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.LARGE_NAMES)
def test_builder_writes_the_models_bytes(ctx, name):
    depth, vox = FAMILIES[name]
    assert_built_is_model(ctx, vox, depth, model(name))


def test_builder_writes_the_models_bytes_for_the_small_subsets(ctx):
    for name in SMALL:
        depth, vox = FAMILIES[name]
        assert_built_is_model(ctx, vox, depth, model(name))


# ---- b. dirty lists --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.DIRTY_NAMES)
def test_builder_ignores_and_resolves_dirty_rows(ctx, name):
    depth, dirty, clean = tc.dirty_case(name)
    assert_built_is_model(ctx, dirty, depth, tree_model.build_cells(clean, depth))


@pytest.mark.parametrize("depth", [1, 4, 10])
def test_a_list_of_dropped_rows_is_one_empty_cell(ctx, depth):
    vbo, n = rt.octree_build_cells(ctx, tc.all_dropped(depth), depth)
    got = vbo.read(np.uint32)
    assert n == 1 and got.size == 16 and not got.any()


# ---- c. the walk against the numpy walk, on cells the GPU builder did not make ---------------------------------------
@pytest.mark.parametrize("name", tc.LARGE_NAMES)
def test_walk_of_the_models_cells(ctx, name):
    """Bound exactly sized, and padded with zero cells so that buffer_cells + 2 (the scan length of a level whose frontier
    capacity is the whole buffer's cells + 1) is one scan tile and one item more.  The padded runs take the families of at
    most 2046 cells: all but level-count-edge-* (whose level-6 frontiers are themselves 2047, 2048 and 2049 live items) and
    sparse-d10; a level's capacity reaches cells + 1 only from level 5 on, so they bite on mixed-scan-edge-* (depth 5) and
    on the ladders of depths 6 and 10."""
    depth, vox = FAMILIES[name]
    cells, want = model(name), tc.sort_vox(vox)
    keep = bind(ctx, cells, depth)
    assert_walk_is_numpy(ctx, cells, depth, want)
    n = len(cells) // 16
    for scan_items in (tc.SCAN_TILE, tc.SCAN_TILE + 1):
        if n > scan_items - 2:
            assert n > 2046 and name.startswith(("level-count-edge", "sparse-d10")), "a family lost its padded runs"
            continue
        padded = np.concatenate([cells, np.zeros(16 * (scan_items - 2 - n), np.uint32)])
        keep = bind(ctx, padded, depth)
        assert ctx.octree_census()["buffer_cells"] + 2 == scan_items
        assert_walk_is_numpy(ctx, padded, depth, want)
    del keep


def test_walk_of_the_models_cells_for_the_small_subsets(ctx):
    for name in SMALL:
        depth, vox = FAMILIES[name]
        bind(ctx, model(name), depth)
        assert_walk_is_numpy(ctx, model(name), depth, tc.sort_vox(vox))


# ---- d. shared cells: the frontier retry and the leaf-only retry ----------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.SHARED))
def test_walk_of_shared_cells_through_the_retries(ctx, name):
    """Bound exactly sized, the walk's first attempt overflows its frontier (the chains) or only its leaf records
    (leaf_overflow).  The census walks without leaf records and the extract with them: each goes first once."""
    cells, depth = tc.shared_tree(name)
    want = tc.sort_vox(expand_cells(cells, depth))
    census = census_of(cells, depth)
    assert {k: census[k] for k in ("reachable_cells", "leaf_nodes", "voxels")} == {k: tc.SHARED[name][k] for k in ("reachable_cells", "leaf_nodes", "voxels")}
    bind(ctx, cells, depth)
    assert ctx.octree_census() == census
    got = ctx.octree_extract()
    assert got.shape == want.shape and np.array_equal(got, want)
    bind(ctx, cells, depth)                                            # a fresh binding, the opposite order
    got = ctx.octree_extract()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert ctx.octree_census() == census


# ---- e. compaction to the model's bytes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5", "d10"])
def test_compaction_of_a_scrambled_tree_gives_the_models_bytes(ctx, name):
    depth, vox = tc.scramble_inputs(name)
    canon = tree_model.build_cells(vox, depth)
    scrambled = tc.scramble(canon, depth, np.random.default_rng(9))
    want_vox = tc.sort_vox(vox)
    vbos = bind(ctx, scrambled, depth, counter=12345)
    assert ctx.octree_census() == census_of(scrambled, depth, 12345)
    assert np.array_equal(ctx.octree_extract(), want_vox)              # cells numbered in no breadth-first order, split LEAFs
    n = ctx.octree_compact()
    assert n == len(canon) // 16
    after = vbos[0].read(np.uint32)
    assert after.size == scrambled.size and np.array_equal(after[: len(canon)], canon) and not after[len(canon):].any()
    assert int(vbos["counter"].read(np.uint32)[0]) == n
    assert np.array_equal(ctx.octree_extract(), want_vox)


def test_compaction_of_the_uniform_chain_is_one_cell(ctx):
    """Through the frontier retry, and four levels of merging: 32^3 voxels of one material are the root's eight LEAFs."""
    cells, depth = tc.chain(5, uniform=True)
    vbos = bind(ctx, cells, depth, counter=5)
    assert ctx.octree_compact() == 1
    after = vbos[0].read(np.uint32)
    assert after.size == cells.size and after[:16].reshape(8, 2).tolist() == [[7, tc.LEAF]] * 8 and not after[16:].any()
    assert int(vbos["counter"].read(np.uint32)[0]) == 1
    assert ctx.octree_census() == dict(reachable_cells=1, leaf_nodes=8, voxels=32 ** 3, max_cell=0, buffer_cells=5, counter=1)


# ---- f. what the edit suites rely on: build, bind, extract at depth 10 -----------------------------------------------
def test_depth_10_round_trip(ctx):
    depth, vox = FAMILIES["sparse-d10"]
    built, n = rt.octree_build_cells(ctx, vox, depth)
    bind(ctx, built.read(np.uint32), depth)
    got = ctx.octree_extract()
    assert np.array_equal(got, tc.sort_vox(vox))
    bind(ctx, model("sparse-d10"), depth)
    assert np.array_equal(got, ctx.octree_extract())
