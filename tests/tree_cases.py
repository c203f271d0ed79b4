"""Test inputs for the two roots of the edit suites, the GPU octree builder (tdt_octree_build_cells) and the GPU tree walk
(tdt_octree_census / tdt_octree_extract / tdt_octree_compact): voxel lists aimed at the builder's level capacities, scan tiles
and merge rule, lists with rows it must ignore or resolve, hand-made trees with shared cells that overflow the walk's frontier
and leaf-record capacities, and canonical trees made non-canonical.  Plain numpy: nothing here touches the GPU or a library.
tests/test_tree_cases.py proves every precondition stated here; tests/test_gpu_tree_roots.py runs the GPU code on the inputs."""
import functools

import numpy as np

EMPTY, PARENT, LEAF = 0, 1, 2
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
SCAN_TILE = 2048                              # device_scan.hpp kScanTile: items of one scan tile


def morton(xyz):
    """Morton key of (n, 3) coordinates below 2^10: the 3-bit digits are x*4 + y*2 + z, most significant level first."""
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    k = np.zeros(len(p), np.int64)
    for b in range(10):
        k |= (((p[:, 0] >> b) & 1) << (3 * b + 2)) | (((p[:, 1] >> b) & 1) << (3 * b + 1)) | (((p[:, 2] >> b) & 1) << (3 * b))
    return k


def sort_vox(v):
    """The list in Morton order (what tdt_octree_extract returns), as contiguous int32."""
    v = np.asarray(v, np.int32).reshape(-1, 4)
    return np.ascontiguousarray(v[np.argsort(morton(v[:, :3]), kind="stable")])


def _unravel(idx, g):
    idx = np.asarray(idx, np.int64)
    return np.stack([idx // (g * g), (idx // g) % g, idx % g], 1)


def _with_materials(rng, xyz, lo=1, hi=254):
    """xyz with random materials lo..hi, both ends used when there are two voxels or more, in random file order."""
    m = rng.integers(lo, hi + 1, size=len(xyz))
    if len(xyz) >= 2:
        m[0], m[1] = lo, hi
    v = np.concatenate([np.asarray(xyz, np.int64), m[:, None]], 1).astype(np.int32)
    return np.ascontiguousarray(v[rng.permutation(len(v))])


def random_voxels(rng, depth, n):
    """n distinct random voxels of the 2^depth grid."""
    g = 1 << depth
    idx = rng.permutation(g ** 3)[:n] if depth <= 7 else np.unique(rng.integers(0, g ** 3, size=2 * n + 64))
    idx = idx[rng.permutation(len(idx))][:n]
    assert len(idx) == n
    return _with_materials(rng, _unravel(idx, g))


def cube(base, side, material):
    """The (side^3, 4) int64 voxels of the cube at `base`."""
    g = np.stack(np.meshgrid(*([np.arange(side)] * 3), indexing="ij"), -1).reshape(-1, 3) + np.asarray(base, np.int64)
    return np.concatenate([g, np.full((len(g), 1), material, np.int64)], 1)


# ---- the merge ladder ------------------------------------------------------------------------------------------------
LADDER_VARIANTS = ("complete", "missing", "other", "offset")


def ladder_block(base, k, variant, material, other):
    """One rung: the block of side 2^k at the 2^k-aligned `base`.  complete: all of one material (one LEAF at its own level);
    missing: without one voxel, not a corner of the grid (k >= 1); other: one voxel of material `other` (k >= 1); offset: the
    block moved by 2^(k-1) on every axis, so that it is eight aligned blocks of side 2^(k-1) under eight different parents."""
    side = 1 << k
    base = np.asarray(base, np.int64)
    assert (base % side == 0).all() and (variant == "complete" or k >= 1)
    if variant == "offset":
        return cube(base + side // 2, side, material)
    v = cube(base, side, material)
    odd = (v[:, :3] == base + [side - 1, 0, 0]).all(1)              # the far end of the block's first row
    assert odd.sum() == 1
    if variant == "missing":
        return v[~odd]
    if variant == "other":
        v[odd, 3] = other
    return v


def _ladder_places(depth, variant):
    """(k, base) per rung: each in a 32^3 region of its own; k = 5 at the origin, k = 4 in the far corner of the grid."""
    h = 1 << (depth - 6)                                          # regions are 32 wide; the far half of the grid starts at h regions
    region = {5: (0, 0, 0), 4: (2 * h - 1,) * 3, 3: (h, 0, 0), 2: (0, h, 0), 1: (0, 0, h), 0: (h, h, 0)}
    out = []
    for k in range(6):
        if k == 0 and variant != "complete":
            continue
        base = 32 * np.array(region[k], np.int64)
        if k == 4 and variant != "offset":
            base = base + 16                                      # touches (2^depth - 1,) * 3
        if k == 5 and variant == "offset" and depth == 6:
            continue                                              # [16, 48)^3 runs through every region: a list of its own
        out.append((k, base))
    return out


def ladder(depth, variant):
    """The rungs k = 0..5 of one variant in one list, each with a material of its own (1 and 254 among them)."""
    rng = np.random.default_rng(600 + 10 * depth + LADDER_VARIANTS.index(variant))
    mats = {5: 17, 4: 254, 3: 1, 2: 130, 1: 253, 0: 2}
    v = np.concatenate([ladder_block(base, k, variant, mats[k], 99) for k, base in _ladder_places(depth, variant)])
    return np.ascontiguousarray(v[rng.permutation(len(v))].astype(np.int32))


def ladder_siblings(depth):
    """Per k = 0..3, in a 32^3 region of its own: two complete aligned blocks of side 2^k of ONE material that are neighbours
    under DIFFERENT parents (x = 2^k and x = 2 * 2^k: they must not merge with each other), and two of different materials
    under one parent."""
    rng = np.random.default_rng(650 + depth)
    h = 1 << (depth - 6)
    region = {0: (0, 0, 0), 1: (2 * h - 1,) * 3, 2: (h, 0, 0), 3: (0, h, 0)}
    out = []
    for k in range(4):
        s, base = 1 << k, 32 * np.array(region[k], np.int64)
        out += [cube(base + [s, 0, 0], s, 40 + k), cube(base + [2 * s, 0, 0], s, 40 + k)]
        out += [cube(base + [0, 16, 0], s, 1), cube(base + [s, 16, 0], s, 254)]
    v = np.concatenate(out)
    return np.ascontiguousarray(v[rng.permutation(len(v))].astype(np.int32))


# ---- the families ----------------------------------------------------------------------------------------------------
def sparse_d10():
    """16 385 random voxels over the whole 1024^3 grid (one past eight sort tiles), plus its eight corners."""
    rng = np.random.default_rng(1010)
    n = 1 << 10
    corners = np.array([[x, y, z] for x in (0, n - 1) for y in (0, n - 1) for z in (0, n - 1)], np.int64)
    idx = np.unique(rng.integers(0, n ** 3, size=40000))
    xyz = _unravel(idx[rng.permutation(len(idx))], n)
    xyz = xyz[~np.isin(morton(xyz), morton(corners))][:16385]
    assert len(xyz) == 16385
    return _with_materials(rng, np.concatenate([corners, xyz]))


def _small_subsets():
    """depth-1: all 255 non-empty subsets of the eight voxels; depth-2: 64 random subsets of the 64, of several densities."""
    rng = np.random.default_rng(12)
    for mask in range(1, 256):
        xyz = np.array([[c >> 2, (c >> 1) & 1, c & 1] for c in range(8) if (mask >> c) & 1], np.int64)
        v = np.concatenate([xyz, rng.integers(1, 3, size=(len(xyz), 1))], 1).astype(np.int32)
        yield f"depth-1-{mask:03d}", 1, np.ascontiguousarray(v[rng.permutation(len(v))])
    all64 = _unravel(np.arange(64), 4)
    for i in range(64):
        keep = rng.random(64) < (0.3, 0.6, 0.9, 1.0)[i % 4]
        keep[int(rng.integers(0, 64))] = True
        xyz = all64[keep]
        m = 1 + (rng.random(len(xyz)) < (0.1, 0.5)[(i // 4) % 2]).astype(np.int64)
        v = np.concatenate([xyz, m[:, None]], 1).astype(np.int32)
        yield f"depth-2-{i:02d}", 2, np.ascontiguousarray(v[rng.permutation(len(v))])


@functools.lru_cache(maxsize=None)
def _families():
    out = []
    # capacity-N: the builder sizes level l as min(n, 8^l)
    for n in (7, 8, 9, 63, 64, 65, 511, 512, 513, 4095):
        out.append((f"capacity-{n}", 4, random_voxels(np.random.default_rng(400 + n), 4, n)))
    rng = np.random.default_rng(404)
    full = _unravel(np.arange(4096), 16)
    out.append(("capacity-4096-full", 4, _with_materials(rng, full)))                  # no level merges
    out.append(("capacity-4096-uniform", 4, _with_materials(rng, full, 254, 254)))     # one cell
    one = _with_materials(rng, full, 9, 9)
    out.append(("capacity-4095-uniform-but-one-missing", 4, np.ascontiguousarray(one[1:])))
    other = one.copy()
    other[0, 3] = 1
    out.append(("capacity-4096-uniform-but-one-other", 4, other))
    # mixed-scan-edge: capacities of levels 1..4 are 8 + 64 + 512 + n, so the MIXED-flag scan runs over 2048 and 2049 items
    for n in (1463, 1464):
        out.append((f"mixed-scan-edge-{n}", 5, random_voxels(np.random.default_rng(500 + n), 5, n)))
    # level-count-edge: one voxel in each of K level-5 blocks, so the head-flag scans run over K + 1 items
    for K in (2047, 2048, 2049):
        rng = np.random.default_rng(550 + K)
        blocks = _unravel(rng.permutation(32 ** 3)[:K], 32)
        out.append((f"level-count-edge-{K}", 6, _with_materials(rng, blocks * 2 + rng.integers(0, 2, size=(K, 3)))))
    for depth in (6, 10):
        for variant in LADDER_VARIANTS:
            out.append((f"merge-ladder-d{depth}-{variant}", depth, ladder(depth, variant)))
        out.append((f"merge-ladder-d{depth}-siblings", depth, ladder_siblings(depth)))
    out.append(("merge-ladder-d6-offset-5", 6, ladder_block((0, 0, 0), 5, "offset", 77, 0).astype(np.int32)))
    out.append(("sparse-d10", 10, sparse_d10()))
    out.extend(_small_subsets())
    for _, _, v in out:
        v.setflags(write=False)
    return tuple(out)


def families():
    """(name, depth, vox): vox (n, 4) int32 {x, y, z, material + 1}, unique positions, random file order, fixed seeds."""
    return _families()


def family(name):
    return next(f for f in _families() if f[0] == name)


def is_small(name):
    """The depth-1 and depth-2 subsets: hundreds of tiny lists, which share one test function each."""
    return name.startswith(("depth-1-", "depth-2-"))


LARGE_NAMES = tuple(n for n, _, _ in _families() if not is_small(n))


# ---- dirty lists -----------------------------------------------------------------------------------------------------
def clean_np(vox, depth):
    """What the builder must make of a list: rows outside the grid or with material + 1 outside 1..254 dropped, and of the
    rows left at one position the last in file order kept; in the order of those last rows."""
    v = np.asarray(vox, np.int64).reshape(-1, 4)
    ok = ((v[:, :3] >= 0) & (v[:, :3] < (1 << depth))).all(1) & (v[:, 3] >= 1) & (v[:, 3] <= 254)
    v = v[ok]
    last = {}
    for i, p in enumerate(map(tuple, v[:, :3])):
        last[p] = i
    return np.ascontiguousarray(v[sorted(last.values())].astype(np.int32))


def dirty(vox, depth, rng):
    """(dirty, clean): `vox` with rows added that the builder must ignore or resolve, in random file order, and what is left.
    Ignored: coordinates -1, 2^depth, INT32_MIN and INT32_MAX on each axis, and material + 1 of 0, 255, 256 and -1 (on free
    positions, and on kept positions anywhere in the file: a dropped row erases nothing).  Resolved: every kept voxel stands
    twice, the earlier copy under another material at an unrelated file position, so the last copy must win."""
    vox = np.asarray(vox, np.int32).reshape(-1, 4)
    n, g = len(vox), 1 << depth
    junk = []
    probe = vox[rng.integers(0, n, size=4)] if n else np.zeros((4, 4), np.int32) + [0, 0, 0, 1]
    for a in range(3):
        for j, c in enumerate((-1, g, INT32_MIN, INT32_MAX)):
            row = probe[j].astype(np.int64)
            row[a] = c
            junk.append(row)
    for m in (0, 255, 256, -1):
        junk.append(np.array([*rng.integers(0, g, size=3), m], np.int64))
        if n:
            junk.append(np.array([*vox[int(rng.integers(0, n))][:3], m], np.int64))
    junk = np.array(junk, np.int64)
    early = vox.astype(np.int64)
    early[:, 3] = (early[:, 3] - 1 + rng.integers(1, 254, size=n)) % 254 + 1           # another material in 1..254
    assert n == 0 or ((early[:, 3] != vox[:, 3]) & (early[:, 3] >= 1) & (early[:, 3] <= 254)).all()
    total = 2 * n + len(junk)
    pos = rng.permutation(total)
    pair = np.sort(pos[: 2 * n].reshape(n, 2), axis=1)            # file positions of the two copies, the earlier first
    out = np.zeros((total, 4), np.int64)
    out[pair[:, 0]] = early
    out[pair[:, 1]] = vox
    out[pos[2 * n:]] = junk
    clean = np.ascontiguousarray(vox[np.argsort(pair[:, 1])])      # the kept rows, in file order
    return np.ascontiguousarray(out.astype(np.int32)), clean


def all_dropped(depth):
    """A list whose every row is dropped."""
    g = 1 << depth
    return np.array([[-1, 0, 0, 1], [0, g, 0, 2], [0, 0, INT32_MAX, 3], [INT32_MIN, 0, 0, 4], [0, 0, 0, 0], [1, 1, 1, 255],
                     [g - 1, 0, 0, 256], [0, g - 1, 0, -1], [g, g, g, 255]], np.int32)


DIRTY_NAMES = ("capacity-9", "capacity-513", "capacity-4096-full", "mixed-scan-edge-1464", "level-count-edge-2048",
               "merge-ladder-d6-other", "merge-ladder-d10-complete", "sparse-d10", "depth-1-255", "depth-2-03")


def dirty_case(name):
    """(depth, dirty, clean) of a family, from a seed fixed by its name."""
    _, depth, vox = family(name)
    d, c = dirty(vox, depth, np.random.default_rng(7000 + DIRTY_NAMES.index(name)))
    return depth, d, c


# ---- trees with shared cells -----------------------------------------------------------------------------------------
def _cells(n):
    return np.zeros((n, 8, 2), np.uint32)


def chain(D, uniform=False):
    """D cells, depth D: all eight nodes of cell i are PARENTs of cell i + 1; the last holds eight LEAFs, values 3..10 or all 7.
    Level l has 8^(l-1) frontier items; bound exactly sized, the walk's frontier capacity is D + 1."""
    c = _cells(D)
    for i in range(D - 1):
        c[i, :, 0], c[i, :, 1] = i + 1, PARENT
    c[D - 1, :, 0] = 7 if uniform else np.arange(3, 11)
    c[D - 1, :, 1] = LEAF
    return c.reshape(-1), D


def deep_chain():
    """Six cells, depth 6: cells 0 and 1 have one PARENT each (nodes 5 and 2), cells 2..4 eight, cell 5 eight LEAFs.  Frontiers
    1, 1, 1, 8, 64, 512 against a capacity of 7: the first overflow is at level 4."""
    c = _cells(6)
    c[0, 5] = [1, PARENT]
    c[1, 2] = [2, PARENT]
    for i in (2, 3, 4):
        c[i, :, 0], c[i, :, 1] = i + 1, PARENT
    c[5, :, 0], c[5, :, 1] = np.arange(20, 28), LEAF
    return c.reshape(-1), 6


def leaf_overflow():
    """Three cells, depth 3.  Frontiers 1, 4, 4 fit the capacity of 4; the 4 + 28 + 32 = 64 leaf records do not fit the
    room of 8 * 4 = 32 the walk starts with: the retry that changes the leaf capacity alone."""
    c = _cells(3)
    c[0, :4, 0], c[0, :4, 1] = 1, PARENT
    c[0, 4:, 0], c[0, 4:, 1] = np.arange(50, 54), LEAF
    c[1, 0] = [2, PARENT]
    c[1, 1:, 0], c[1, 1:, 1] = np.arange(60, 67), LEAF
    c[2, :, 0], c[2, :, 1] = np.arange(70, 78), LEAF
    return c.reshape(-1), 3


# expected numbers of the shared-cell trees (tests/test_tree_cases.py asserts them with the numpy walk)
SHARED = {
    "chain5": dict(frontiers=[1, 8, 64, 512, 4096], reachable_cells=4681, leaf_nodes=32768, voxels=32768),
    "chain6": dict(frontiers=[1, 8, 64, 512, 4096, 32768], reachable_cells=37449, leaf_nodes=262144, voxels=262144),
    "deep_chain": dict(frontiers=[1, 1, 1, 8, 64, 512], reachable_cells=587, leaf_nodes=4096, voxels=4096),
    "leaf_overflow": dict(frontiers=[1, 4, 4], reachable_cells=9, leaf_nodes=64, voxels=512),
}


def shared_tree(name):
    return {"chain5": lambda: chain(5), "chain6": lambda: chain(6), "deep_chain": deep_chain, "leaf_overflow": leaf_overflow}[name]()


def frontiers(cells, depth):
    """Frontier items per level of the walk (a shared cell counts once per path), and leaf records in all."""
    c = np.asarray(cells, np.uint32).reshape(-1, 8, 2)
    f, sizes, leaves = np.zeros(1, np.int64), [], 0
    for level in range(1, depth + 1):
        sizes.append(int(f.size))
        nodes = c[f]
        leaves += int((nodes[..., 1] == LEAF).sum())
        f = nodes[..., 0][nodes[..., 1] == PARENT].astype(np.int64) if level < depth else np.zeros(0, np.int64)
    return sizes, leaves


# ---- scrambled trees -------------------------------------------------------------------------------------------------
def scramble(cells, depth, rng, split_cap=64, dead=5):
    """A non-canonical tree of the same voxels as the canonical `cells`: up to split_cap LEAFs above the finest level become
    PARENTs of new cells of eight identical LEAFs, `dead` unreachable cells of random words with types 0..2 are appended, and
    all cells but cell 0 are renumbered by a random permutation (PARENT values fixed up), so the numbering is not breadth-first."""
    c = np.asarray(cells, np.uint32).reshape(-1, 8, 2).copy()
    # the level of every cell: breadth-first from cell 0 (canonical trees are trees: one path per cell)
    level = np.zeros(len(c), np.int64)
    level[0] = 1
    for i in range(len(c)):                                        # canonical numbering: a parent comes before its children
        kids = c[i, :, 0][c[i, :, 1] == PARENT]
        level[kids] = level[i] + 1
    ci, ni = np.nonzero((c[..., 1] == LEAF) & (level[:, None] < depth))
    pick = rng.permutation(len(ci))[:split_cap]
    fresh = np.zeros((len(pick), 8, 2), np.uint32)
    for j, p in enumerate(pick):
        fresh[j, :, 0], fresh[j, :, 1] = c[ci[p], ni[p], 0], LEAF
        c[ci[p], ni[p]] = [len(c) + j, PARENT]
    junk = np.zeros((dead, 8, 2), np.uint32)
    junk[..., 0] = rng.integers(0, 1 << 32, size=(dead, 8), dtype=np.uint64).astype(np.uint32)
    junk[..., 1] = rng.integers(0, 3, size=(dead, 8))
    c = np.concatenate([c, fresh, junk])
    new_of = np.concatenate([[0], 1 + rng.permutation(len(c) - 1)])            # old cell number -> new
    live = np.ones(len(c), bool)
    live[len(c) - dead:] = False
    par = (c[..., 1] == PARENT) & live[:, None]
    c[..., 0][par] = new_of[c[..., 0][par]].astype(np.uint32)
    out = np.zeros_like(c)
    out[new_of] = c
    return np.ascontiguousarray(out.reshape(-1))


def scramble_inputs(name):
    """(depth, vox) of the two lists whose canonical trees get scrambled: d5 = 3 000 random voxels of the depth-5 grid plus
    aligned 2^3 and 4^3 blocks; d10 = sparse-d10 plus a 32^3 block."""
    if name == "d5":
        rng = np.random.default_rng(55)
        blocks = [cube((4, 8, 12), 4, 200), cube((28, 28, 28), 4, 1), cube((16, 0, 4), 4, 254)]
        blocks += [cube(2 * np.array(b), 2, 30 + i) for i, b in enumerate([(0, 0, 0), (15, 0, 15), (7, 3, 9), (1, 14, 6), (12, 5, 0), (9, 9, 3)])]
        blocks = np.concatenate(blocks)
        loose = random_voxels(rng, 5, 3000).astype(np.int64)
        loose = loose[~np.isin(morton(loose[:, :3]), morton(blocks[:, :3]))]
        v = np.concatenate([loose, blocks])
        return 5, np.ascontiguousarray(v[rng.permutation(len(v))].astype(np.int32))
    rng = np.random.default_rng(1055)
    block = cube((512, 256, 768), 32, 11)
    loose = sparse_d10().astype(np.int64)
    loose = loose[~np.isin(morton(loose[:, :3]), morton(block[:, :3]))]
    v = np.concatenate([loose, block])
    return 10, np.ascontiguousarray(v[rng.permutation(len(v))].astype(np.int32))
