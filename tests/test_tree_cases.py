"""tests/tree_cases.py makes the inputs of tests/test_gpu_tree_roots.py; this proves, without a GPU, that they are what they
claim: the two numpy models (tree_model.build_cells and octree_util.expand_cells) invert each other on every list, depth 10
included, and every count, capacity and overflow the GPU tests aim at is really there."""
import numpy as np
import pytest

import tree_cases as tc
import tree_model
from octree_util import expand_cells
from test_gpu_octree_compact import census_np

FAMILIES = {name: (depth, vox) for name, depth, vox in tc.families()}
SMALL = [n for n in FAMILIES if tc.is_small(n)]


def rebuilt(vox, depth):
    return tc.sort_vox(expand_cells(tree_model.build_cells(vox, depth), depth))


def n_cells(vox, depth):
    return len(tree_model.build_cells(vox, depth)) // 16


# ---- the lists -------------------------------------------------------------------------------------------------------
def check_list(vox, depth):
    assert vox.dtype == np.int32 and vox.ndim == 2 and vox.shape[1] == 4 and len(vox) >= 1
    assert ((vox[:, :3] >= 0) & (vox[:, :3] < (1 << depth))).all() and ((vox[:, 3] >= 1) & (vox[:, 3] <= 254)).all()
    assert len(np.unique(tc.morton(vox[:, :3]))) == len(vox), "a position stands twice"
    assert np.array_equal(rebuilt(vox, depth), tc.sort_vox(vox))


@pytest.mark.parametrize("name", tc.LARGE_NAMES)
def test_the_two_models_invert_each_other(name):
    depth, vox = FAMILIES[name]
    check_list(vox, depth)
    if len(vox) > 64 and not name.startswith("merge-ladder"):
        assert (np.diff(tc.morton(vox[:, :3])) < 0).any(), "the file order is the Morton order"


def test_the_two_models_invert_each_other_on_the_small_subsets():
    assert len(SMALL) == 255 + 64
    for name in SMALL:
        check_list(FAMILIES[name][1], FAMILIES[name][0])
        assert set(FAMILIES[name][1][:, 3].tolist()) <= {1, 2}


def test_both_ends_of_the_material_range_are_used():
    for name in tc.LARGE_NAMES:
        if name.startswith(("capacity-4096-uniform", "capacity-4095-uniform", "merge-ladder-d6-offset-5")):
            continue
        m = FAMILIES[name][1][:, 3]
        assert m.min() == 1 and m.max() == 254, name


def test_capacity_families():
    """Level l of the builder holds min(n, 8^l) entries: n straddles 8, 64 and 512, and the full grid fills every level."""
    for n in (7, 8, 9, 63, 64, 65, 511, 512, 513, 4095):
        depth, vox = FAMILIES[f"capacity-{n}"]
        assert depth == 4 and len(vox) == n
    depth, full = FAMILIES["capacity-4096-full"]
    cells = tree_model.build_cells(full, depth).reshape(-1, 8, 2)
    assert len(full) == 4096 and len(cells) == 1 + 8 + 64 + 512 and (cells[..., 1] != tc.EMPTY).all()
    assert [tree_model.parents_at_level(cells, l) for l in (1, 2, 3)] == [8, 64, 512]           # no level merges
    depth, uni = FAMILIES["capacity-4096-uniform"]
    assert tree_model.build_cells(uni, depth).reshape(8, 2).tolist() == [[253, tc.LEAF]] * 8   # one cell
    for name, n in (("capacity-4095-uniform-but-one-missing", 4095), ("capacity-4096-uniform-but-one-other", 4096)):
        depth, vox = FAMILIES[name]
        cells = tree_model.build_cells(vox, depth).reshape(-1, 8, 2)
        assert len(vox) == n and len(cells) == 4                                               # one cell per level, one path
        assert [tree_model.parents_at_level(cells, l) for l in (1, 2, 3, 4)] == [1, 1, 1, 0]
        assert ((cells[..., 1] == tc.LEAF).sum(1) >= 7).all()


def test_scan_edge_families():
    for n, items in ((1463, tc.SCAN_TILE), (1464, tc.SCAN_TILE + 1)):
        depth, vox = FAMILIES[f"mixed-scan-edge-{n}"]
        assert depth == 5 and len(vox) == n
        assert sum(min(n, 8 ** l) for l in range(1, depth)) + 1 == items       # the MIXED-flag scan: levels 1..4 end to end, + 1
    for K in (2047, 2048, 2049):
        depth, vox = FAMILIES[f"level-count-edge-{K}"]
        assert depth == 6 and len(vox) == K
        assert len(np.unique(tc.morton(vox[:, :3] >> 1))) == K                 # one voxel per level-5 block: K heads, K + 1 flags
        cells = tree_model.build_cells(vox, depth)
        assert tc.frontiers(cells, depth)[0][-1] == K and len(cells) // 16 > K # and the walk's last frontier is K live items


def test_which_families_the_padded_walks_take():
    """The GPU walk test pads a family's cells to 2046 and 2047 cells where they fit: every depth must be among those."""
    fits = [n for n in tc.LARGE_NAMES if n_cells(FAMILIES[n][1], FAMILIES[n][0]) <= tc.SCAN_TILE - 2]
    assert {FAMILIES[n][0] for n in fits} == {4, 5, 6, 10}
    assert sorted(set(tc.LARGE_NAMES) - set(fits)) == ["level-count-edge-2047", "level-count-edge-2048", "level-count-edge-2049", "sparse-d10"]


def test_sparse_d10():
    depth, vox = FAMILIES["sparse-d10"]
    assert depth == 10 and len(vox) == 16385 + 8
    have = set(map(tuple, vox[:, :3].tolist()))
    assert all((x, y, z) in have for x in (0, 1023) for y in (0, 1023) for z in (0, 1023))
    assert tree_model.parents_at_level(tree_model.build_cells(vox, 10), 9) > 0


def test_small_subsets():
    masks = set()
    for name in SMALL:
        depth, vox = FAMILIES[name]
        if depth == 1:
            masks.add(sum(1 << int(4 * x + 2 * y + z) for x, y, z in vox[:, :3]))
    assert masks == set(range(1, 256))
    merged = 0
    for name in SMALL:
        depth, vox = FAMILIES[name]
        if depth == 2:
            for o in range(8):
                inside = vox[(tc.morton(vox[:, :3]) >> 3) == o]
                if len(inside) == 8 and len(set(inside[:, 3].tolist())) == 1:
                    merged += 1
                    root = tree_model.build_cells(vox, 2).reshape(-1, 8, 2)[0, o]
                    assert root.tolist() == [inside[0, 3] - 1, tc.LEAF]        # a level-1 LEAF
    assert merged >= 1


# ---- the merge ladder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [6, 10])
def test_merge_ladder_cell_counts_by_hand(depth):
    """A complete aligned block of side 2^k is one LEAF at level depth - k: it costs the depth - k cells of its path and none
    below.  Without one voxel, or with one of another material, the path goes on to the finest level: exactly k more cells."""
    far = (1 << depth) - 32
    for k in range(6):
        base = (far, 0, far) if k % 2 else (0, far, 0)
        assert n_cells(tc.ladder_block(base, k, "complete", 5, 6), depth) == depth - k
        if k == 0:
            continue
        assert n_cells(tc.ladder_block(base, k, "missing", 5, 6), depth) == depth
        assert n_cells(tc.ladder_block(base, k, "other", 5, 6), depth) == depth
        # the offset block: eight LEAFs of side 2^(k-1), under eight parents
        inner = tuple(max(b - 32, 0) for b in base)                           # (the moved block must stay inside the grid)
        cells = tree_model.build_cells(tc.ladder_block(inner, k, "offset", 5, 6), depth)
        c = census_np(cells, depth)
        assert (c["leaf_nodes"], c["voxels"]) == (8, 8 ** k)
        assert tree_model.parents_at_level(cells, depth - k) == 8


@pytest.mark.parametrize("depth", [6, 10])
def test_merge_ladder_families(depth):
    n = (1 << depth) - 1
    rungs = {"complete": range(6), "missing": range(1, 6), "other": range(1, 6), "offset": range(1, 5 if depth == 6 else 6)}
    cells_of = {}
    for variant, ks in rungs.items():
        d, vox = FAMILIES[f"merge-ladder-d{depth}-{variant}"]
        assert d == depth
        have = set(map(tuple, vox[:, :3].tolist()))
        if variant != "offset":
            assert (0, 0, 0) in have and (n, n, n) in have               # one block touches the origin, one the far corner
        want = sum(8 ** k for k in ks) - (len(ks) if variant == "missing" else 0)
        assert len(vox) == want
        cells_of[variant] = tree_model.build_cells(vox, depth)
        c = census_np(cells_of[variant], depth)
        if variant == "complete":
            assert c["leaf_nodes"] == 6                                   # every block one LEAF
        if variant == "offset":
            assert c["leaf_nodes"] == 8 * len(ks)                         # every block eight smaller LEAFs
    # rung k = 0 of the complete list costs cells of its own; without it the difference is the k more cells of each rung
    d, vox = FAMILIES[f"merge-ladder-d{depth}-complete"]
    no_k0 = vox[vox[:, 3] != 2]
    assert len(no_k0) == len(vox) - 1
    assert len(cells_of["missing"]) // 16 - n_cells(no_k0, depth) == 1 + 2 + 3 + 4 + 5
    assert len(cells_of["other"]) == len(cells_of["missing"])
    # siblings: four blocks per k, none merged with a neighbour, none split
    d, vox = FAMILIES[f"merge-ladder-d{depth}-siblings"]
    c = census_np(tree_model.build_cells(vox, depth), depth)
    assert (c["leaf_nodes"], c["voxels"]) == (16, 4 * (1 + 8 + 64 + 512)) and len(vox) == c["voxels"]
    for k in range(4):                                                    # the same-material pair really has two parents
        pair = vox[vox[:, 3] == 40 + k]
        assert len(pair) == 2 * 8 ** k and len(np.unique(tc.morton(pair[:, :3]) >> (3 * k))) == 2
        assert len(np.unique(tc.morton(pair[:, :3]) >> (3 * k + 3))) == 2
        low = pair[:, 0].min()
        assert set((pair[:, 0] - low).tolist()) == set(range(2 << k))      # neighbours along x


# ---- dirty lists -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.DIRTY_NAMES)
def test_dirty_lists(name):
    depth, vox = FAMILIES[name]
    d2, dirty, clean = tc.dirty_case(name)
    g = 1 << depth
    assert d2 == depth and dirty.dtype == np.int32 and len(dirty) == 2 * len(vox) + 12 + 8
    assert np.array_equal(clean, tc.clean_np(dirty, depth))               # keep the last copy per position, drop the rest
    assert np.array_equal(tc.sort_vox(clean), tc.sort_vox(vox))
    assert np.array_equal(rebuilt(clean, depth), tc.sort_vox(vox))
    for a in range(3):
        assert {-1, g, tc.INT32_MIN, tc.INT32_MAX} <= set(dirty[:, a].tolist())
    assert {0, 255, 256, -1} <= set(dirty[:, 3].tolist())
    # the earlier copy of every kept voxel carries another material: first-wins or any-wins would give another tree
    key = tc.morton(clean[:, :3])
    ok = ((dirty[:, :3] >= 0) & (dirty[:, :3] < g)).all(1) & (dirty[:, 3] >= 1) & (dirty[:, 3] <= 254)
    valid = dirty[ok]
    first = {}
    for row in valid[::-1]:
        first[tuple(row[:3])] = row[3]
    assert all(first[tuple(row[:3])] != row[3] for row in clean)
    assert len(valid) == 2 * len(clean) and len(np.unique(key)) == len(clean)


def test_all_dropped_list():
    for depth in (1, 4, 10):
        assert len(tc.all_dropped(depth)) >= 9 and len(tc.clean_np(tc.all_dropped(depth), depth)) == 0


# ---- trees with shared cells -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.SHARED))
def test_shared_cell_trees(name):
    cells, depth = tc.shared_tree(name)
    want = tc.SHARED[name]
    sizes, leaves = tc.frontiers(cells, depth)
    assert sizes == want["frontiers"] and leaves == want["leaf_nodes"]
    c = census_np(cells, depth)
    assert {k: c[k] for k in ("reachable_cells", "leaf_nodes", "voxels")} == {k: want[k] for k in ("reachable_cells", "leaf_nodes", "voxels")}
    assert c["buffer_cells"] == len(cells) // 16 == (depth if name != "leaf_overflow" else 3) and c["max_cell"] == c["buffer_cells"] - 1
    assert len(expand_cells(cells, depth)) == want["voxels"]
    # what the walk starts with, bound exactly sized: frontier capacity min(8^(l-1), cells + 1), leaf room 8 per frontier item
    room = c["buffer_cells"] + 1
    cap = [min(8 ** l, room) for l in range(depth)]
    over = [l + 1 for l in range(depth) if sizes[l] > cap[l]]
    leaf_room = min(8 * room, 8 * sum(cap))
    if name == "leaf_overflow":
        assert not over and room == 4 and leaf_room == 32 < leaves == 64      # the leaf-only retry
    else:
        assert over[0] == {"chain5": 2, "chain6": 2, "deep_chain": 4}[name]    # the frontier retry, from that level on
        assert room == depth + 1


def test_uniform_chain_is_one_block():
    cells, depth = tc.chain(5, uniform=True)
    vox = expand_cells(cells, depth)
    assert len(vox) == 32 ** 3 and (vox[:, 3] == 8).all()
    assert tree_model.build_cells(vox, depth).reshape(8, 2).tolist() == [[7, tc.LEAF]] * 8


# ---- scrambled trees -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_vox", [("d5", 3000), ("d10", 16000 + 32768)])
def test_scramble(name, n_vox):
    depth, vox = tc.scramble_inputs(name)
    check_list(vox, depth)
    assert len(vox) >= n_vox
    canon = tree_model.build_cells(vox, depth)
    s =tc.scramble(canon, depth, np.random.default_rng(9))
    assert s.dtype == np.uint32 and len(s) > len(canon) and not np.array_equal(s[: len(canon)], canon)
    assert len(s) // 16 - len(canon) // 16 > 5                         # split cells were added beside the dead ones
    assert np.array_equal(tc.sort_vox(expand_cells(s, depth)), tc.sort_vox(vox))
    assert np.array_equal(tree_model.build_cells(expand_cells(s, depth), depth), canon)
    # the numbering is not breadth-first: the PARENT values met by the walk are not 1, 2, 3, ...
    c = s.reshape(-1, 8, 2)
    f, seen = np.zeros(1, np.int64), []
    for _ in range(depth):
        nodes = c[f]
        f = nodes[..., 0][nodes[..., 1] == tc.PARENT].astype(np.int64)
        seen.append(f)
    seen = np.concatenate(seen)
    assert len(np.unique(seen)) == len(seen) and (np.diff(seen) < 0).any()
    assert len(seen) + 1 == len(c) - 5                                  # every cell but the five dead ones is reached once
