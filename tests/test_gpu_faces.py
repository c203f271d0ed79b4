"""Face tools (tdt_octree_face_regions / tdt_octree_extract_faces / tdt_octree_edit_faces): the face list, the labels and the region
table must equal the numpy model (tests/faces_model.py) bit for bit, with and without the hook stage's in-wave pre-merge; the face
list must equal tdt_octree_extract_surface(merge = 0) on the GPU; the column list must equal the model's; the edit form must leave
in the bound cells buffer exactly the builder's tree of op(V, column list) followed by zeros."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import faces_model as fm
import surface_model as sm
from test_gpu_connect import bind_tree, block
from test_gpu_region_edit import apply_op, bind_cells, built_cells, expected_bytes, morton, padded, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

pytestmark = pytest.mark.gpu
OPS = (rt.REGION_SET, rt.REGION_FILL, rt.REGION_PAINT, rt.REGION_CLEAR)
KINDS = [(c, m) for c in (4, 8) for m in (rt.MATCH_ANY, rt.MATCH_MATERIAL)]


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def check_regions(ctx, V, depth, regions=None, kinds=KINDS, tag=""):
    """F, labels and table against the model for every kind, with and without the pre-merge; F against the surface extraction.
    Returns (F, {kind: (labels, table)}) of the model."""
    F = fm.face_list(V, depth, regions)
    Q = fm.quads(F)
    surface = ctx.octree_extract_surface(merge=False, regions=regions)
    assert surface.shape == Q.shape and np.array_equal(surface, Q), tag
    out = {}
    for conn, match in kinds:
        want_l, want_t = fm.face_regions(F, depth, conn, match)
        out[(conn, match)] = (want_l, want_t)
        try:
            for premerge in (True, False):
                ctx.debug_faces_premerge(premerge)
                faces, labels, tab = ctx.octree_face_regions(conn, match, regions, capacity=max(len(F), 1))
                assert faces.shape == Q.shape and np.array_equal(faces, Q), (tag, conn, match, premerge)
                assert labels.dtype == np.uint32 and np.array_equal(labels, want_l), (tag, conn, match, premerge)
                assert tab.dtype == want_t.dtype and len(tab) == len(want_t) and tab.tobytes() == want_t.tobytes(), (tag, conn, match, premerge)
        finally:
            ctx.debug_faces_premerge(True)
    return F, out


def check_columns(ctx, V, depth, seeds, distance, tag="", **kw):
    want = fm.column_list(V, depth, seeds, distance, **kw)
    got = ctx.octree_extract_faces(seeds, distance, rt.FACES_COLUMNS, **kw)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (tag, distance, kw)
    tree = ctx.octree_extract_faces(seeds, distance, rt.FACES_TREE, **kw)
    assert np.array_equal(tree, fm.intersect(V, want)), (tag, distance, kw)
    return want


def plate(mask2d, z, m=1):
    """A one-voxel-thick plate in the plane z: the voxels (x, y, z) where mask2d[x, y]."""
    p = np.argwhere(mask2d)
    return np.concatenate([p, np.full((len(p), 1), z), np.full((len(p), 1), m)], 1).astype(np.int32)


# ---- 1. random trees -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 5, 6])
def test_regions_of_random_trees_equal_the_model(ctx, depth):
    rng = np.random.default_rng(300 + depth)
    n = 1 << depth
    occ = rng.random((n, n, n)) < (0.55 if depth < 6 else 0.3)
    occ[n // 4: n // 2, n // 4: n // 2, n // 4: n // 2] = True                # a solid block: larger flat regions among the noise
    mat = rng.integers(1, 4, (n, n, n))
    vbo, counter, V = bind_tree(ctx, sm.grid_voxels(occ, mat), depth)
    before = vbo.read(np.uint32)
    F, res = check_regions(ctx, V, depth, tag=f"random{depth}")
    counts = {k: len(t) for k, (_, t) in res.items()}
    assert counts[(8, rt.MATCH_ANY)] < counts[(4, rt.MATCH_ANY)] < counts[(4, rt.MATCH_MATERIAL)] < len(F)
    assert counts[(8, rt.MATCH_ANY)] < counts[(8, rt.MATCH_MATERIAL)] < counts[(4, rt.MATCH_MATERIAL)]
    assert max(t["faces"].max() for _, t in res.values()) > 8
    assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345     # it only reads
    # seeds on some of them, both directions of the distance, blocked and not
    pick = rng.choice(len(F), 6, replace=False)
    seeds = np.array([[*V[F[i, fm.OWNER_], :3], F[i, fm.F_]] for i in pick], np.int32)
    for conn, match in KINDS:
        for d, blocked, material in ((2, False, -1), (-2, True, 5), (n, True, -1)):
            want = check_columns(ctx, V, depth, seeds, d, connectivity=conn, match=match, block=blocked, material=material, tag=f"random{depth}")
            assert len(want) > 0


# ---- 2. launch boundaries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257])
def test_face_counts_at_launch_boundaries(ctx, count):
    depth, n = 5, 32
    m2 = np.zeros(n * n, bool)
    m2[:count] = True                                              # rows of 32 along y, filled in raster order
    V = sort_vox(plate(m2.reshape(n, n), 7, 3))
    F = fm.face_list(V, depth)
    assert (F[:, fm.F_] == 4).sum() == count and (F[:, fm.F_] == 5).sum() == count
    bind_tree(ctx, V, depth)
    _, res = check_regions(ctx, V, depth, tag=count)
    _, tab = res[(4, rt.MATCH_ANY)]
    assert tab[tab["face"] == 5]["faces"].tolist() == [count]
    want = check_columns(ctx, V, depth, [[0, 0, 7, 5]], 2, tag=count)
    assert len(want) == 2 * count


def spiral(n):
    """A one-cell-wide square spiral on an n x n board, walls between its turns: one 4-connected path from the rim to the middle."""
    m = np.zeros((n, n), bool)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = True
    while True:
        nx, ny = x + dx, y + dy
        ahead2 = (nx + dx, ny + dy)
        blocked = not (0 <= nx < n and 0 <= ny < n) or m[nx, ny] or (0 <= ahead2[0] < n and 0 <= ahead2[1] < n and m[ahead2])
        if blocked:
            dx, dy = -dy, dx
            nx, ny = x + dx, y + dy
            ahead2 = (nx + dx, ny + dy)
            if not (0 <= nx < n and 0 <= ny < n) or m[nx, ny] or (0 <= ahead2[0] < n and 0 <= ahead2[1] < n and m[ahead2]):
                return m
        x, y = nx, ny
        m[x, y] = True


def comb(n):
    """A spine along x = n - 1 with a tooth on every other row: the teeth meet only at the far end of the v order."""
    m = np.zeros((n, n), bool)
    m[n - 1, :] = True
    m[:, ::2] = True
    return m


def test_one_region_over_many_blocks_and_long_union_chains(ctx):
    depth, n = 6, 64
    wall = np.ones((n, n), bool)
    checker = (np.add.outer(np.arange(n), np.arange(n)) % 2) == 0
    V = sort_vox(np.concatenate([plate(wall, 3, 2), plate(spiral(n), 20, 4), plate(comb(n), 30, 5), plate(checker, 40, 6)]))
    F = fm.face_list(V, depth)
    # what the case claims, by the model alone
    _, t4 = fm.face_regions(F, depth, 4, rt.MATCH_ANY)
    _, t8 = fm.face_regions(F, depth, 8, rt.MATCH_ANY)
    up4, up8 = t4[t4["face"] == 5], t8[t8["face"] == 5]
    assert up4[up4["w"] == 3]["faces"].tolist() == [n * n]                       # the wall: one region over 16 blocks of 256 lanes
    sp = int(spiral(n).sum())
    assert sp > n * n // 3 and up4[up4["w"] == 20]["faces"].tolist() == [sp]     # the spiral: one chain, its root at the rim
    assert up4[up4["w"] == 30]["faces"].tolist() == [int(comb(n).sum())]
    assert (up4[up4["w"] == 40]["faces"] == 1).all() and (up4["w"] == 40).sum() == n * n // 2
    assert up8[up8["w"] == 40]["faces"].tolist() == [n * n // 2]                 # the checkerboard: all joined by corners
    bind_tree(ctx, V, depth)
    check_regions(ctx, V, depth, tag="planes")
    want = check_columns(ctx, V, depth, [[0, 0, 20, 5], [0, 0, 40, 4]], 3, connectivity=8, tag="planes")
    assert len(want) == 3 * (sp + n * n // 2)


# ---- 3. grid edges ---------------------------------------------------------------------------------------------------------------
def test_regions_at_the_grid_edges(ctx):
    depth, n = 4, 16
    V = sort_vox(np.concatenate([block((0, 0, 0), (n - 1, n - 1, 0), 1), block((0, 0, n - 1), (3, n - 1, n - 1), 2),
                                 block((n - 1, 0, 5), (n - 1, n - 1, 9), 3), block((0, n - 1, 5), (5, n - 1, 9), 4)]))
    bind_tree(ctx, V, depth)
    F, res = check_regions(ctx, V, depth, tag="edges")
    _, tab = res[(4, rt.MATCH_MATERIAL)]
    assert (tab["lo"] == 0).any() and (tab["hi"] == n - 1).any()
    # regions on the grid's own faces: their pull is clipped to nothing, their push runs inwards
    for seed in ([3, 3, 0, 4], [n - 1, 3, 7, 1], [2, n - 1, 7, 3], [0, 3, n - 1, 0]):
        assert check_columns(ctx, V, depth, [seed], 5, tag=seed).shape == (0, 4)
        assert check_columns(ctx, V, depth, [seed], rt.FACES_DISTANCE_MAX, block=True, tag=seed).shape == (0, 4)
        assert len(check_columns(ctx, V, depth, [seed], -2, tag=seed)) > 0
    vbo, counter = bind_cells(ctx, ctx._keep[0].read(np.uint32), 600)
    want, n_cells = expected_bytes(ctx, V, depth, 64 * 600)
    assert ctx.octree_edit_faces(rt.REGION_FILL, [[3, 3, 0, 4]], 7) == n_cells and np.array_equal(vbo.read(np.uint32), want)


def test_depth_ten_keys_that_differ_by_one_are_not_neighbours(ctx):
    depth = 10
    vox = np.array([[5, 7, 1023, 1], [5, 8, 0, 1],              # +-x faces: (w 5, u 7, v 1023) and (w 5, u 8, v 0): keys differ by 1
                    [1023, 50, 7, 1], [0, 50, 8, 1],            # +-y faces: (w 50, u 7, v 1023) and (w 50, u 8, v 0)
                    [7, 1023, 90, 1], [8, 0, 90, 1],            # +-z faces: (w 90, u 7, v 1023) and (w 90, u 8, v 0)
                    [200, 1023, 3, 1], [201, 0, 3, 1],          # +-x faces: (w 200, u 1023, v 3) and (w 201, u 0, v 3): key + 1024 carries into w
                    [300, 300, 1022, 1], [300, 300, 1023, 1], [300, 301, 1023, 1]], np.int32)   # real neighbours at the edge, for contrast
    vbo, counter, V = bind_tree(ctx, vox, depth)
    F = fm.face_list(V, depth)
    keys = (F[:, fm.W_] << 20) | (F[:, fm.U_] << 10) | F[:, fm.V_]
    for f in range(6):
        k = keys[F[:, fm.F_] == f]
        assert (np.diff(k) == 1).sum() >= (2 if f < 2 else 1)                     # the carry pair (and for +-x the real pair along v)
    _, res = check_regions(ctx, V, depth, tag="depth10")
    for kind, (labels, tab) in res.items():
        pairs = {(int(t["face"]), int(t["w"])): int(t["faces"]) for t in tab}
        for f, w in ((0, 5), (1, 5), (2, 50), (3, 50), (4, 90), (5, 90), (0, 200), (1, 200), (0, 201), (1, 201)):
            assert (tab[(tab["face"] == f) & (tab["w"] == w)]["faces"] == 1).all(), (kind, f, w)
        assert ((tab["face"] == 1) & (tab["w"] == 5)).sum() == 2 and pairs[(1, 300)] == 3
    want = check_columns(ctx, V, depth, [[5, 7, 1023, 1]], 3, connectivity=8, match=rt.MATCH_ANY, tag="depth10")
    assert want[:, :3].tolist() == [[6, 7, 1023], [7, 7, 1023], [8, 7, 1023]]


# ---- 4. the mask confines ---------------------------------------------------------------------------------------------------------
def test_mask_confines_a_region(ctx):
    depth = 4
    V = sort_vox(block((0, 0, 6), (15, 15, 7), 2))
    bind_tree(ctx, V, depth)
    mask = [rt.box((0, 0, 0), (6, 15, 15)), rt.sphere((12, 12, 7), 2)]
    F, res = check_regions(ctx, V, depth, regions=mask, tag="mask")
    _, tab = res[(4, rt.MATCH_ANY)]
    top = tab[tab["face"] == 5]
    assert sorted(top["faces"].tolist()) == [13, 7 * 16]                         # the wall's part under the box, and the disc: two regions
    want = check_columns(ctx, V, depth, [[2, 2, 7, 5]], 2, regions=mask, tag="mask")
    assert len(want) == 2 * 7 * 16 and want[:, 0].max() == 6
    assert check_columns(ctx, V, depth, [[9, 2, 7, 5]], 2, regions=mask, tag="mask").shape == (0, 4)     # a seed outside the mask
    assert len(check_columns(ctx, V, depth, [[9, 2, 7, 5]], 2, tag="no mask")) == 2 * 256
    assert check_columns(ctx, V, depth, [[2, 2, 7, 5]], 2, regions=[], tag="empty mask").shape == (0, 4)


# ---- 5. seeds ----------------------------------------------------------------------------------------------------------------------
def test_seeds(ctx):
    depth = 4
    V = sort_vox(np.concatenate([block((2, 2, 2), (6, 6, 6), 1), block((9, 9, 2), (12, 12, 4), 2), block((2, 10, 10), (3, 11, 11), 3)]))
    bind_tree(ctx, V, depth)
    check_regions(ctx, V, depth, tag="seeds")
    nothing = [[8, 8, 8, 1], [16, 3, 3, 1], [-1, 3, 3, 0], [3, 3, 1024, 5], [4, 4, 4, 1], [6, 4, 4, 0], [6, 4, 4, 2]]   # air, off the grid, buried
    for s in nothing:
        assert check_columns(ctx, V, depth, [s], 2, tag=s).shape == (0, 4)
    assert check_columns(ctx, V, depth, nothing, -3, tag="nothing").shape == (0, 4)
    one = check_columns(ctx, V, depth, [[6, 4, 4, 1]], 2)
    assert len(one) == 50
    dup = check_columns(ctx, V, depth, [[6, 4, 4, 1], [6, 2, 6, 1], [6, 4, 4, 1]] + nothing, 2)        # duplicates, the same region twice
    assert np.array_equal(dup, one)
    many = check_columns(ctx, V, depth, [[6, 4, 4, 1], [4, 4, 6, 5], [9, 10, 3, 0], [3, 11, 10, 3], [2, 2, 2, 2]], 2, material=7)
    assert len(many) > 3 * len(one) // 2 and (many[:, 3] == 8).all()


# ---- 6. columns --------------------------------------------------------------------------------------------------------------------
def test_columns(ctx):
    depth = 4
    slab = block((4, 2, 2), (6, 11, 11), 1)                         # 3 thick along x
    slab[(slab[:, 1] + slab[:, 2]) % 3 == 0, 3] = 2                 # two colours over the wall
    obstacle = block((9, 4, 4), (9, 7, 7), 5)                       # 2 voxels of air away from the slab's +x face
    V = sort_vox(np.concatenate([slab, obstacle]))
    bind_tree(ctx, V, depth)
    seed = [[6, 5, 5, 1]]
    for d in (1, -1, 3, -3, rt.FACES_DISTANCE_MAX, -rt.FACES_DISTANCE_MAX):
        for blocked in (False, True):
            for material in (-1, 0, 253):
                check_columns(ctx, V, depth, seed, d, match=rt.MATCH_ANY, block=blocked, material=material)
    free = check_columns(ctx, V, depth, seed, 1023, match=rt.MATCH_ANY)
    assert len(free) == 100 * 9 and set(free[:, 3]) == {1, 2}                    # x = 7 .. 15, the wall's colours continued
    stopped = check_columns(ctx, V, depth, seed, 1023, match=rt.MATCH_ANY, block=True)
    assert len(stopped) == 100 * 9 - 16 * 7                                      # the 16 columns under the obstacle end after 2
    assert (stopped[(stopped[:, 1] == 5) & (stopped[:, 2] == 5), 0].tolist()) == [7, 8]
    through = check_columns(ctx, V, depth, seed, -1023, match=rt.MATCH_ANY)
    assert len(through) == 100 * 7                                               # x = 6 .. 0: block = 0 passes through the slab
    carved = check_columns(ctx, V, depth, seed, -1023, match=rt.MATCH_ANY, block=True)
    assert len(carved) == 300 and carved[:, 0].min() == 4                        # the push stops at the air behind the slab
    # MATCH_MATERIAL: only the faces of the seed's colour
    part = check_columns(ctx, V, depth, seed, 2, match=rt.MATCH_MATERIAL)
    assert 0 < len(part) < 200 and set(part[:, 3]) == {int(V[(V[:, :3] == [6, 5, 5]).all(1), 3][0])}


@pytest.mark.parametrize("gap", [3, 4])
def test_overlapping_columns_take_the_later_direction(ctx, gap):
    depth = 4
    left, right = block((2, 4, 4), (3, 7, 7), 3), block((4 + gap, 4, 4), (5 + gap, 7, 7), 8)
    V = sort_vox(np.concatenate([left, right]))
    bind_tree(ctx, V, depth)
    seeds = [[4 + gap, 5, 5, 0], [3, 5, 5, 1]]
    B = check_columns(ctx, V, depth, seeds, gap)
    assert len(B) == 16 * gap and (B[:, 3] == 3).all()
    half = check_columns(ctx, V, depth, seeds[::-1], (gap + 1) // 2)
    assert set(half[:, 3]) == {3, 8}
    # one direction at different w: two plates behind each other pulled the same way; the higher w comes later in F
    V = sort_vox(np.concatenate([block((2, 4, 4), (3, 7, 7), 3), block((6, 4, 4), (7, 7, 7), 9)]))
    bind_tree(ctx, V, depth)
    B = check_columns(ctx, V, depth, [[7, 5, 5, 1], [3, 5, 5, 1]], 6)
    assert len(B) == 16 * 10 and (B[B[:, 0] <= 7, 3] == 3).all() and (B[B[:, 0] >= 8, 3] == 9).all()


# ---- 7. the edit and extract forms -------------------------------------------------------------------------------------------------
def test_every_op_equals_edit_voxels_of_the_column_list(ctx):
    depth = 5
    rng = np.random.default_rng(77)
    centres = rng.integers(4, 28, (24, 3))
    vox = np.concatenate([block(c - rng.integers(1, 4, 3), c + rng.integers(1, 4, 3), int(rng.integers(1, 9))) for c in centres])
    vox = vox[((vox[:, :3] >= 0) & (vox[:, :3] < 32)).all(1)]
    _, first = np.unique(morton(vox[:, :3]), return_index=True)
    vbo, counter, V = bind_tree(ctx, vox[np.sort(first)], depth)
    cells = vbo.read(np.uint32)
    F = fm.face_list(V, depth)
    labels, tab = fm.face_regions(F, depth, 4, rt.MATCH_MATERIAL)
    big = np.argsort(tab["faces"])[-3:]
    seeds = np.array([[*V[F[tab["first"][r], fm.OWNER_], :3], tab["face"][r]] for r in big], np.int32)
    for d, blocked, material in ((3, False, -1), (-2, False, 6), (-1, False, 11), (9, True, -1)):
        B = fm.column_list(V, depth, seeds, d, block=blocked, material=material)
        assert len(B) > 0
        for op in OPS:
            want_vox = apply_op(V, op, B, 0)
            assert np.array_equal(want_vox, fm.edit(V, depth, op, seeds, d, block=blocked, material=material))
            built = built_cells(ctx, want_vox, depth)
            n_want = len(built) // 16
            room = max(len(cells) // 16, n_want) + 8
            vbo, counter = bind_cells(ctx, cells, room)
            n = ctx.octree_edit_faces(op, seeds, d, block=blocked, material=material)
            got = vbo.read(np.uint32)
            assert n == n_want and int(counter.read(np.uint32)[0]) == n, (d, op)
            assert np.array_equal(got, padded(built, 64 * room)), (d, op)
            vbo, counter = bind_cells(ctx, cells, room)
            assert ctx.octree_edit_voxels(op, ctx.octree_extract_faces(seeds, d, rt.FACES_COLUMNS, block=blocked, material=material)) == n
            assert np.array_equal(vbo.read(np.uint32), got), (d, op)
    # the undo record of a push: TDT_FACES_TREE, the edit, then SET of the record restores the bytes
    room = 8 ** depth // 7 + 2                                      # no depth-5 tree has more cells
    vbo, counter = bind_cells(ctx, cells, room)
    saved = ctx.octree_extract_faces(seeds, -3, rt.FACES_TREE)
    assert 0 < len(saved) < len(V) and np.array_equal(saved, fm.extract(V, depth, seeds, -3, fm.TREE))
    assert np.array_equal(vbo.read(np.uint32), padded(cells, 64 * room)) and int(counter.read(np.uint32)[0]) == 12345      # extract writes nothing
    canonical, n0 = expected_bytes(ctx, V, depth, 64 * room)
    ctx.octree_edit_faces(rt.REGION_CLEAR, seeds, -3)
    assert not np.array_equal(vbo.read(np.uint32), canonical)
    assert ctx.octree_edit_voxels(rt.REGION_SET, saved) == n0
    assert np.array_equal(vbo.read(np.uint32), canonical)
    # an empty selection installs the compacted bytes: no seeds, distance 0, a seed on air
    for s, d in ((np.zeros((0, 4), np.int32), 3), (seeds, 0), ([[31, 31, 31, 1]], 3)):
        vbo, counter = bind_cells(ctx, cells, room)
        assert ctx.octree_edit_faces(rt.REGION_SET, s, d) == n0 and np.array_equal(vbo.read(np.uint32), canonical)
        assert ctx.octree_extract_faces(s, d).shape == (0, 4)


def test_a_misfit_reports_the_cells_and_keeps_the_bytes(ctx):
    depth = 5
    vbo, counter, V = bind_tree(ctx, block((8, 8, 8), (15, 15, 15), 4), depth)     # a few merged cells
    chain = vbo.read(np.uint32)
    seed = [[15, 9, 9, 1]]
    built = built_cells(ctx, fm.edit(V, depth, rt.REGION_FILL, seed, 3), depth)
    need = len(built) // 16
    assert need > len(chain) // 16
    vbo, counter = bind_cells(ctx, chain, need - 1)
    with pytest.raises(rt.TdtError) as e:
        ctx.octree_edit_faces(rt.REGION_FILL, seed, 3)
    assert e.value.code == rt.ERR_INVALID_VALUE and e.value.n_cells == need
    assert np.array_equal(vbo.read(np.uint32), padded(chain, 64 * (need - 1))) and int(counter.read(np.uint32)[0]) == 12345
    vbo, counter = bind_cells(ctx, chain, need)
    assert ctx.octree_edit_faces(rt.REGION_FILL, seed, 3) == need and np.array_equal(vbo.read(np.uint32), built)


def extrude_scene():
    base = host.Scene.config(2)                                    # what the demo program draws in the suites' demo tests
    depth = base.max_depth
    room = 8 ** depth // 7 + 2                                      # no depth-6 tree has more cells
    return host.Scene({**base.blobs, 0: padded(np.ascontiguousarray(base.blobs[0]).view(np.uint32), 64 * room)}), depth, room


def hit_pixel(r, w, h):
    """The pixel nearest the middle of the frame whose pick yields a seed, and that seed."""
    uniforms = (r.vbos[6].read(np.float32), r.vbos[7].read(np.int32))
    px = np.array([[x, y] for y in range(h // 4, 3 * h // 4, 3) for x in range(w // 4, 3 * w // 4, 3)], np.int32)
    px = px[np.argsort(np.abs(px - [w // 2, h // 2]).sum(1), kind="stable")]
    for p, hit in zip(px, r.pick(px)):
        try:
            return p, host.pick_face(hit, uniforms)
        except ValueError:
            continue
    raise AssertionError("no pixel of the frame hits the model")


def test_two_member_context_edits_both_replicas(oracle):
    w, h = 96, 64
    scene, depth, room = extrude_scene()
    cam = host.camera_reference_pose(w, h, 2, 3)
    outs = []
    for devices in (None, [0, 0]):                                 # two members on one device: every replica path, on any machine
        r = rt.Renderer(scene, cam, devices=devices)
        try:
            r.render()
            pixel, seed = hit_pixel(r, w, h)
            cols = r.ctx.octree_extract_faces(seed, 3, material=5)
            faces, labels, tab = r.ctx.octree_face_regions(capacity=1 << 16)
            before = r.vbos[0].read(np.uint32)
            bad = rt.Faces(4, rt.MATCH_MATERIAL, 3, 0, 254, 0)
            nc = ctypes.c_uint32(0)
            assert rt.lib().tdt_octree_edit_faces(r.ctx.h, rt.REGION_SET, ctypes.byref(bad), seed.ctypes.data, 1, None, 0,
                                                  ctypes.byref(nc)) == rt.ERR_INVALID_VALUE
            assert np.array_equal(r.vbos[0].read(np.uint32), before)
            V = r.ctx.octree_extract()
            n = r.ctx.octree_edit_faces(rt.REGION_SET, seed, 3, material=5)
            outs.append((n, r.vbos[0].read(np.uint32), r.render(), V, cols, labels, tab, seed))
        finally:
            r.close()
    (n1, c1, img1, V1, l1, lab1, t1, s1), (n2, c2, img2, V2, l2, lab2, t2, s2) = outs
    assert n1 == n2 and np.array_equal(c1, c2) and np.array_equal(l1, l2) and np.array_equal(lab1, lab2) and t1.tobytes() == t2.tobytes()
    assert np.array_equal(s1, s2) and len(l1) > 0 and np.array_equal(l1, fm.column_list(V1, depth, s1, 3, material=5))
    ctx2 = rt.Context(0)
    try:
        want, n = expected_bytes(ctx2, apply_op(V1, rt.REGION_SET, l1, 0), depth, 64 * room)
    finally:
        ctx2.close()
    assert n1 == n and np.array_equal(c1, want) and not np.array_equal(c1, np.ascontiguousarray(scene.blobs[0]).view(np.uint32))
    assert (img1.view(np.uint32) == img2.view(np.uint32)).all()
    ref = oracle.render(host.Scene({**scene.blobs, 0: c2}), cam, threads=4)
    assert (img2.view(np.uint32) == ref.view(np.uint32)).all()


# ---- 8. through the renderer -------------------------------------------------------------------------------------------------------
def test_renderer_extrude_then_render(oracle):
    """Scene.demo() stands for 235 M voxels whose canonical tree no test can afford (tests/test_gpu_stroke.py), so the renderer's
    form runs on config 2, the scene the demo program draws in the suites' demo tests."""
    w, h = 96, 64
    scene, depth, room = extrude_scene()
    cam = host.camera_reference_pose(w, h, 2, 3)
    r = rt.Renderer(scene, cam)
    try:
        r.render()
        pixel, seed = hit_pixel(r, w, h)
        uniforms = (r.vbos[6].read(np.float32), r.vbos[7].read(np.int32))
        assert np.array_equal(seed, host.pick_face(r.pick([pixel])[0], uniforms))
        V = r.ctx.octree_extract()
        B = fm.column_list(V, depth, seed, 4, material=9)
        assert len(B) > 0
        got_seed, cells = r.extrude(pixel, 4, rt.REGION_FILL, material=9)
        assert got_seed.dtype == np.int32 and np.array_equal(got_seed, seed)
        got = r.vbos[0].read(np.uint32)
        frames = [r.render(), r.render()]
        rim = np.array([[x, y] for x in range(w) for y in (0, h - 1)] + [[x, y] for y in range(h) for x in (0, w - 1)], np.int32)
        sky = rim[r.pick(rim)["status"] != rt.RAY_HIT]
        assert len(sky) > 0
        with pytest.raises(ValueError):
            r.extrude(sky[0], 4, rt.REGION_FILL)                                   # the sky: a miss
        assert np.array_equal(r.vbos[0].read(np.uint32), got)
    finally:
        r.close()
    ctx2 = rt.Context(0)
    try:
        want, n = expected_bytes(ctx2, apply_op(V, rt.REGION_FILL, B, 0), depth, 64 * room)
    finally:
        ctx2.close()
    assert cells == n and np.array_equal(got, want) and not np.array_equal(got, np.ascontiguousarray(scene.blobs[0]).view(np.uint32))
    ref = oracle.render(host.Scene({**scene.blobs, 0: got}), cam, threads=4)
    for img in frames:
        assert (img.view(np.uint32) == ref.view(np.uint32)).all()


def test_demo_extrude_equals_the_python_call(tmp_path):
    exe = build.build_demo()
    w, h = 96, 64
    scene, depth, room = extrude_scene()
    cam = host.camera_reference_pose(w, h, 2, 3)                   # the demo's camera
    r = rt.Renderer(scene, cam)
    try:
        pixel, seed = hit_pixel(r, w, h)
        _, n = r.extrude(pixel, 3, rt.REGION_FILL, material=6, connectivity=8, match=rt.MATCH_ANY, block=True)
        img = r.render()
    finally:
        r.close()
    out = str(tmp_path / "extrude.pfm")
    p = subprocess.run([exe, "--config", "2", "--size", f"{w}x{h}", "--spp", "2", "--bounce", "3", "--cells", str(room), "--pick",
                        f"{pixel[0]},{pixel[1]}", "--extrude", "3", "--conn", "8", "--block", "1", "--op", "fill", "--material", "6", "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"extrude seed (-?\d+),(-?\d+),(-?\d+) face (\d) distance (-?\d+) op (\w+) cells (\d+)", p.stdout)
    assert m, p.stdout
    assert [int(m.group(i)) for i in range(1, 5)] == seed.tolist() and int(m.group(5)) == 3 and m.group(6) == "fill" and int(m.group(7)) == n
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF4"
        fw, fh = map(int, f.readline().split())
        f.readline()
        frame = np.frombuffer(f.read(), "<f4").reshape(fh, fw, 4)
    assert (frame.view(np.uint32) == img.view(np.uint32)).all()


# ---- 9. errors leave every byte as it was --------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    L = rt.lib()
    scene = host.Scene.config(2)
    depth = scene.max_depth
    cells = np.ascontiguousarray(scene.blobs[0]).view(np.uint32)
    nc, nv, nf, nr = ctypes.c_uint32(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    ctx = rt.Context(0)
    try:
        ok = rt.Faces(4, rt.MATCH_MATERIAL, 2, 0, -1, 0)
        seed = np.array([[1, 2, 3, 1]], np.int32)
        # unbound slots
        for bound in ((), (0,), (7,)):
            for s in bound:
                b = rt.VertexBufferObject(ctx, cells if s == 0 else np.array([depth, 64, 128], np.int32))
                ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, s, b)
            assert L.tdt_octree_edit_faces(ctx.h, 0, ctypes.byref(ok), seed.ctypes.data, 1, None, 0, ctypes.byref(nc)) == rt.ERR_INCOMPLETE
            for what in (rt.FACES_COLUMNS, rt.FACES_TREE):
                assert L.tdt_octree_extract_faces(ctx.h, ctypes.byref(ok), seed.ctypes.data, 1, None, 0, what, None, 0, ctypes.byref(nv)) == rt.ERR_INCOMPLETE
            assert L.tdt_octree_face_regions(ctx.h, 4, 0, None, 0, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nr)) == rt.ERR_INCOMPLETE
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 0, None)
            ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 7, None)
        vbos = rt.upload_scene(ctx, scene)
        counter = rt.VertexBufferObject(ctx, np.array([777], np.uint32))
        ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, counter)
        V = ctx.octree_extract()
        F = fm.face_list(V, depth)
        _, tab4 = fm.face_regions(F, depth, 4, rt.MATCH_MATERIAL)
        first = int(tab4["first"][np.argmax(tab4["faces"])])                       # a face of the largest region
        seed = np.array([[*V[F[first, fm.OWNER_], :3], F[first, fm.F_]]], np.int32)
        cols = fm.column_list(V, depth, seed, 2)
        assert len(cols) > 1

        def unchanged():
            return np.array_equal(vbos[0].read(np.uint32), cells) and int(counter.read(np.uint32)[0]) == 777

        def raw(**f):
            s = rt.Faces(4, rt.MATCH_MATERIAL, 2, 0, -1, 0)
            for k, v in f.items():
                setattr(s, k, v)
            return s

        out = np.zeros((4096, 4), np.int32)
        bad_shape = rt.Region(2, (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(5, 5, 5), 0)
        bad_sphere = rt.sphere((3, 3, 3), -1)
        seed6, seedm = seed.copy(), seed.copy()
        seed6[0, 3], seedm[0, 3] = 6, -1
        calls = [(raw(connectivity=6), seed, 1, None, 0), (raw(connectivity=0), seed, 1, None, 0), (raw(connectivity=26), seed, 1, None, 0),
                 (raw(match=2), seed, 1, None, 0), (raw(match=-1), seed, 1, None, 0),
                 (raw(distance=1024), seed, 1, None, 0), (raw(distance=-1024), seed, 1, None, 0),
                 (raw(block=2), seed, 1, None, 0), (raw(block=-1), seed, 1, None, 0),
                 (raw(material=254), seed, 1, None, 0), (raw(material=-2), seed, 1, None, 0), (raw(pad=1), seed, 1, None, 0),
                 (ok, None, 1, None, 0),                                        # NULL seeds with a count above 0
                 (ok, seed, 1, None, 1),                                        # NULL regions with a count above 0
                 (ok, seed6, 1, None, 0), (ok, seedm, 1, None, 0),              # a seed f outside 0..5
                 (ok, seed, (1 << 20) + 1, None, 0),                            # more than 2^20 seeds (refused before any is read)
                 (ok, seed, 1, ctypes.byref(bad_shape), 1), (ok, seed, 1, ctypes.byref(bad_sphere), 1)]
        for i, (f, s, ns, reg, nreg) in enumerate(calls):
            sp = s.ctypes.data if s is not None else None
            for rc in (L.tdt_octree_edit_faces(ctx.h, rt.REGION_SET, ctypes.byref(f), sp, ns, reg, nreg, ctypes.byref(nc)),
                       L.tdt_octree_extract_faces(ctx.h, ctypes.byref(f), sp, ns, reg, nreg, rt.FACES_COLUMNS, out.ctypes.data, len(out), ctypes.byref(nv)),
                       L.tdt_octree_extract_faces(ctx.h, ctypes.byref(f), sp, ns, reg, nreg, rt.FACES_TREE, out.ctypes.data, len(out), ctypes.byref(nv))):
                assert rc == rt.ERR_INVALID_VALUE and unchanged() and not out.any() and nv.value == 0, i
        sp = seed.ctypes.data
        for rc in (L.tdt_octree_edit_faces(ctx.h, rt.REGION_SET, None, sp, 1, None, 0, ctypes.byref(nc)),                     # a NULL struct
                   L.tdt_octree_edit_faces(ctx.h, 4, ctypes.byref(ok), sp, 1, None, 0, ctypes.byref(nc)),                     # a bad op
                   L.tdt_octree_edit_faces(ctx.h, -1, ctypes.byref(ok), sp, 1, None, 0, ctypes.byref(nc)),
                   L.tdt_octree_extract_faces(ctx.h, None, sp, 1, None, 0, 0, None, 0, ctypes.byref(nv)),
                   L.tdt_octree_extract_faces(ctx.h, ctypes.byref(ok), sp, 1, None, 0, 2, None, 0, ctypes.byref(nv)),         # what out of range
                   L.tdt_octree_extract_faces(ctx.h, ctypes.byref(ok), sp, 1, None, 0, -1, None, 0, ctypes.byref(nv)),
                   L.tdt_octree_extract_faces(ctx.h, ctypes.byref(ok), sp, 1, None, 0, 0, None, 0, None),
                   L.tdt_octree_face_regions(ctx.h, 6, 0, None, 0, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nr)),
                   L.tdt_octree_face_regions(ctx.h, 4, 2, None, 0, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nr)),
                   L.tdt_octree_face_regions(ctx.h, 4, 0, None, 1, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nr)),
                   L.tdt_octree_face_regions(ctx.h, 4, 0, ctypes.byref(bad_shape), 1, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nr)),
                   L.tdt_octree_face_regions(ctx.h, 4, 0, None, 0, None, None, 0, None, None, 0, ctypes.byref(nr)),
                   L.tdt_octree_face_regions(ctx.h, 4, 0, None, 0, None, None, 0, ctypes.byref(nf), None, 0, None)):
            assert rc == rt.ERR_INVALID_VALUE and unchanged()
        # what the wrapper refuses never reaches the library
        for f in (lambda: ctx.octree_edit_faces(4, seed, 2), lambda: ctx.octree_edit_faces(0, seed, 1024), lambda: ctx.octree_extract_faces(seed, 2, 2),
                  lambda: ctx.octree_face_regions(6), lambda: ctx.octree_edit_faces(0, seed6, 2)):
            with pytest.raises(ValueError):
                f()
        assert unchanged()
        # the list rules: NULL counts only; a capacity below the count: the count, nothing written
        for what, full in ((rt.FACES_COLUMNS, cols), (rt.FACES_TREE, fm.intersect(V, fm.column_list(V, depth, seed, -2)))):
            f = raw(distance=2 if what == rt.FACES_COLUMNS else -2)
            args = (ctypes.byref(f), seed.ctypes.data, 1, None, 0, what)
            assert len(full) > 1
            assert L.tdt_octree_extract_faces(ctx.h, *args, None, 0, ctypes.byref(nv)) == rt.OK and nv.value == len(full)
            buf = np.zeros((len(full), 4), np.int32)
            nv = ctypes.c_size_t(0)
            assert L.tdt_octree_extract_faces(ctx.h, *args, buf.ctypes.data, len(full) - 1, ctypes.byref(nv)) == rt.ERR_INVALID_VALUE
            assert nv.value == len(full) and not buf.any()
            assert L.tdt_octree_extract_faces(ctx.h, *args, buf.ctypes.data, len(full), ctypes.byref(nv)) == rt.OK and np.array_equal(buf, full)
        # tdt_octree_face_regions: NULL arrays only count; a short capacity sets the counts and writes nothing
        labels_m, tab_m = fm.face_regions(F, depth, 4, rt.MATCH_ANY)
        assert L.tdt_octree_face_regions(ctx.h, 4, 0, None, 0, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nr)) == rt.OK
        assert (nf.value, nr.value) == (len(F), len(tab_m))
        q, lab, tab = np.zeros((len(F), 8), np.int32), np.zeros(len(F), np.uint32), np.zeros(len(tab_m), rt.FACE_REGION_DTYPE)
        for fcap, tcap in ((len(F) - 1, len(tab_m)), (len(F), len(tab_m) - 1)):
            nf, nr = ctypes.c_size_t(0), ctypes.c_size_t(0)
            assert L.tdt_octree_face_regions(ctx.h, 4, 0, None, 0, q.ctypes.data, lab.ctypes.data, fcap, ctypes.byref(nf), tab.ctypes.data, tcap,
                                             ctypes.byref(nr)) == rt.ERR_INVALID_VALUE
            assert (nf.value, nr.value) == (len(F), len(tab_m)) and not q.any() and not lab.any() and not tab.tobytes().strip(b"\0")
        assert L.tdt_octree_face_regions(ctx.h, 4, 0, None, 0, None, lab.ctypes.data, len(F), ctypes.byref(nf), None, 0, ctypes.byref(nr)) == rt.OK
        assert np.array_equal(lab, labels_m) and not q.any()
        assert unchanged()
    finally:
        ctx.close()


def test_leaf_value_254_and_the_pair_limit(ctx):
    depth = 4
    vbo, counter, V = bind_tree(ctx, np.array([[3, 3, 3, 1], [3, 3, 4, 1]], np.int32), depth)
    high = vbo.read(np.uint32).copy()
    nodes = high.reshape(-1, 8, 2)
    i, j = np.argwhere(nodes[..., 1] == 2)[0]
    nodes[i, j, 0] = 254                                           # a LEAF value >= 254
    vbo3, counter3 = bind_cells(ctx, high, len(high) // 16)
    before = vbo3.read(np.uint32)
    with pytest.raises(rt.TdtError) as e:
        ctx.octree_face_regions()
    assert e.value.code == rt.ERR_INVALID_VALUE
    for f in (lambda: ctx.octree_extract_faces([[3, 3, 4, 5]], 2), lambda: ctx.octree_extract_faces([[3, 3, 4, 5]], 2, rt.FACES_TREE),
              lambda: ctx.octree_edit_faces(rt.REGION_FILL, [[3, 3, 4, 5]], 2)):
        with pytest.raises(rt.TdtError) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE
    assert np.array_equal(vbo3.read(np.uint32), before) and int(counter3.read(np.uint32)[0]) == 12345
    # the pair limit.  No tree of depth <= 9 can pass it with 1023 steps at most, so: a 1024 x 65 plate on the top face of the
    # depth-10 grid pushed through all 1023 layers below is 66560 * 1023 > 2^26 (face, voxel) pairs; one layer less goes through
    depth = 10
    m2 = np.zeros((1024, 1024), bool)
    m2[:, :65] = True
    vbo, counter, V = bind_tree(ctx, plate(m2, 1023, 1), depth, room=64)
    before = vbo.read(np.uint32)
    total = 1024 * 65 * 1023
    assert total > rt.REGION_BRUSH_CAP >= 1024 * 65 * 1008
    for f in (lambda: ctx.octree_extract_faces([[5, 5, 1023, 5]], -1023), lambda: ctx.octree_edit_faces(rt.REGION_FILL, [[5, 5, 1023, 5]], -1023)):
        with pytest.raises(rt.TdtError, match=str(total)) as e:
            f()
        assert e.value.code == rt.ERR_INVALID_VALUE
    assert np.array_equal(vbo.read(np.uint32), before) and int(counter.read(np.uint32)[0]) == 12345
    assert len(ctx.octree_extract_faces([[5, 5, 1023, 5]], -3)) == 1024 * 65 * 3
