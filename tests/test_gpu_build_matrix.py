"""Every scene-specialised build of the trace kernel (kTraceVariants in csrc/tdt_rt.hip), by name: one case per build that makes
the smallest scene selecting it, asserts that this build ran, and compares its pixels with the oracle bit for bit.

The parity tests do not read last_variant() and test_gpu_variants.py compares no pixels, so a build could serve a tree it was
not meant for, or a scene could drop to the general kernel, with every test green.  Here the octree is placed (never at the
usual corner), the tree really has cells at its finest level, and depth 10 — which the scene generators do not reach — is
rendered in all its rows from trees the numpy builder of tests/tree_model.py makes.

Trees.  A row's tree is a generated scene's voxels on the 2^depth grid, at the grid's min corner.  Where the generator's depth
is the row's depth that is the generated scene itself, cells and all (non-resident rows up to depth 9, resident rows up to
depth 6).  No generated scene of depth 7 or more fits the LDS table (the smallest, a depth-7 terrain, has some 17 000 cells against
5120), and none has depth 10, so those rows embed a shallower scene: config 2 (4209 cells) for the resident rows, config 5
(572 991 cells, cell indices past 2^19) for depth 10 outside the table.  The detail then sits in a corner block of the octree, finest
cells at level `depth`; the cameras stand by that block.

Cameras.  Two per case: the reference pose scaled into the block (inside the octree, looking along -z), and one just outside
the min corner looking along the diagonal, whose rays enter the octree through its three min faces, i.e. exactly at w == min.

Premises (CPU: the oracle and the cells, before the GPU is touched): each camera sees the tree (its image differs from the same
camera's image of an all-EMPTY tree in a fifth of the pixels); rows of depth >= 6 have PARENTs at level depth - 1; and for depth
10 the oracle's image changes in at least 5 % of the pixels when the same buffers are rendered under max_depth = 9."""
import numpy as np
import pytest

import octree_util
import tree_model
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

POW2, TABLE = 1, 2                            # tdt::FORM_POW2, tdt::FORM_TABLE (0: the literal form, which has no specialised build)
W, H, SPP, BOUNCE = 96, 64, 3, 6              # 3 spp: below the two-phase limit, the frame's last launch is the main one

# (form, depth, resident, full, brick): kTraceVariants without its unit column, row for row
ROWS = [
    (POW2, 6, 0, 0, 1), (POW2, 7, 0, 0, 1), (POW2, 8, 0, 0, 1), (POW2, 9, 0, 0, 1), (POW2, 10, 0, 0, 1),
    (POW2, 6, 0, 0, 0), (POW2, 7, 0, 0, 0), (POW2, 8, 0, 0, 0), (POW2, 9, 0, 0, 0), (POW2, 10, 0, 0, 0),
    (POW2, 5, 1, 1, 0), (POW2, 6, 1, 1, 0),
    (POW2, 3, 1, 0, 0), (POW2, 4, 1, 0, 0), (POW2, 5, 1, 0, 0), (POW2, 6, 1, 0, 0),
    (POW2, 7, 1, 0, 0), (POW2, 8, 1, 0, 0), (POW2, 9, 1, 0, 0), (POW2, 10, 1, 0, 0),
    (TABLE, 3, 1, 0, 0), (TABLE, 4, 1, 0, 0), (TABLE, 5, 1, 0, 0), (TABLE, 6, 1, 0, 0),
    (TABLE, 7, 1, 0, 0), (TABLE, 8, 1, 0, 0), (TABLE, 9, 1, 0, 0), (TABLE, 10, 1, 0, 0),
    (TABLE, 6, 0, 0, 0), (TABLE, 7, 0, 0, 0), (TABLE, 8, 0, 0, 0), (TABLE, 9, 0, 0, 0), (TABLE, 10, 0, 0, 0),
]

# the source scene of a row's tree, by (depth, resident): a config number or Scene.generate's (kind, depth, cell_count, max_iter, seed)
SOURCES = {
    (3, 1): 1, (4, 1): (host.SCENE_TERRAIN, 4, 1 << 14, 100, 7), (5, 1): (host.SCENE_TERRAIN, 5, 1 << 14, 100, 7), (6, 1): 2,
    (7, 1): 2, (8, 1): 2, (9, 1): 2, (10, 1): 2,
    (6, 0): (host.SCENE_HASH_GRID, 6, 1 << 16, 100, 7), (7, 0): (host.SCENE_TERRAIN, 7, 1 << 16, 256, 7), (8, 0): 3, (9, 0): 5, (10, 0): 5,
}
LDS_CELLS = 5120                              # csrc/trace_device.hpp kLdsCells
TABLE_COUNTS = (100000, 1000003)              # the reference's own count; a larger one for trees of more cells

UNIT_CORNER = np.array([0.75, -1.5, 0.25], np.float32)
NEG_ZERO = np.array([0x80000000], np.uint32).view(np.float32)[0]
ZERO_CORNERS = [np.array([0.0, -1.5, 0.25], np.float32),                  # min_x = +0
                np.array([0.75, NEG_ZERO, 0.25], np.float32),             # min_y = -0
                np.array([0.0, 0.0, 0.0], np.float32)]

_sources, _trees, _scenes = {}, {}, {}


def _source(spec):
    if spec not in _sources:
        _sources[spec] = host.Scene.config(spec) if isinstance(spec, int) else host.Scene.generate(*spec)
    return _sources[spec]


def _tree(depth, resident):
    """(cells, source scene, edge of the detail block in octree units) of the rows of this depth and residency."""
    key = (depth, resident)
    if key not in _trees:
        src = _source(SOURCES[key])
        if src.max_depth == depth:
            cells = src.blobs[0]
        else:
            cells = tree_model.build_cells(octree_util.expand_cells(src.blobs[0], src.max_depth), depth)
        cells.setflags(write=False)
        _trees[key] = (cells, src, 2.0 ** (src.max_depth - depth))
    return _trees[key]


def _scene(row):
    """The row's scene at the usual corner: its tree under the cell_count that selects the row's form."""
    if row not in _scenes:
        form, depth, resident, _, _ = row
        cells, src, block = _tree(depth, resident)
        n = cells.size // 16
        cc = max(src.cell_count, 1 << int(n).bit_length())                # a power of two above every cell index
        assert cc & (cc - 1) == 0 and n < cc <= 1 << 22
        scene = tree_model.scene_from_cells(cells, depth, cc, src)
        if form == TABLE:
            scene = host.scene_with_cell_count(scene, next(c for c in TABLE_COUNTS if c > n))
        _scenes[row] = (scene, block)
    return _scenes[row]


def _camera(origin, view, fov=90.0):
    """Camera uniforms for an eye at `origin` looking along `view` (camera.rs:135-196's frame, turned): float32 throughout."""
    f32 = np.float32
    d = np.asarray(view, np.float64)
    d = (d / np.linalg.norm(d)).astype(f32)
    right = np.cross(d, np.array([0, 1, 0], f32)).astype(f32)
    right = (right / f32(np.linalg.norm(right))).astype(f32)
    up = np.cross(right, d).astype(f32)
    vh = f32(2.0 * np.tan(np.radians(fov) / 2.0))
    vw = f32(f32(W) / f32(H)) * vh
    o = np.asarray(origin, f32)
    hor, ver = right * vw, up * vh
    llc = o - hor * f32(0.5) - ver * f32(0.5) + d
    u = host.CameraUniforms()
    u.image_width, u.image_height, u.samples_per_pixel, u.max_bounce = W, H, SPP, BOUNCE
    for name, v in (("horizontal", hor), ("vertical", ver), ("lower_left_corner", llc), ("origin", o)):
        getattr(u, name)[:] = [float(x) for x in v.astype(f32)]
    return u


def _cameras(corner, block):
    """Inside: the reference pose (main.rs:165-168: (0.5, 0.4, 0.7) from the corner, looking along -z) scaled into the detail block.
    Outside: just beyond the min corner, looking at the block's middle.  From there the octree lies in the directions with three
    positive components only, so the view is narrow (45 degrees) around the diagonal: every ray that meets the octree enters it
    through a min face."""
    c = corner.astype(np.float32)
    b = np.float32(block)
    inside = _camera(c + b * np.array([0.5, 0.4, 0.7], np.float32), (0.0, 0.0, -1.0))
    eye = np.array([-0.05, -0.05, -0.05], np.float32)
    outside = _camera(c + b * eye, np.array([0.5, 0.4, 0.5]) - eye.astype(np.float64), fov=45.0)
    return inside, outside


def _differ(a, b):
    return float((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).mean())


def _with_ints(scene, **kw):
    blobs = {k: v.copy() for k, v in scene.blobs.items()}
    for k, v in kw.items():
        blobs[7][{"max_depth": 0, "max_iter": 1, "cell_count": 2}[k]] = v
    return host.Scene(blobs, scene.counts, scene.name)


def _case(oracle, row, unit, index):
    """(placed scene, cameras, oracle images) of one build, with its premises checked on the CPU."""
    form, depth, resident, full, brick = row
    scene, block = _scene(row)
    corner = UNIT_CORNER if unit else ZERO_CORNERS[index % 3]
    placed = tree_model.with_corner(scene, corner)
    assert placed.blobs[6][:3].view(np.uint32).tolist() == corner.view(np.uint32).tolist()
    assert placed.blobs[6][4] == 1.0 and placed.blobs[6][5] == 1.0
    assert (corner != 0).all() == bool(unit)
    cells = placed.blobs[0]
    n_cells = cells.size // 16
    live = int(np.flatnonzero(cells.reshape(-1, 2).any(axis=1)).max()) + 1
    values = cells.reshape(-1, 2)[:, 0]
    if resident:
        assert live <= LDS_CELLS * 8 and int(values.max()) <= 0x3FFE
    else:
        assert LDS_CELLS * 8 < live and n_cells <= 1 << 21
    if depth >= 6:
        assert tree_model.parents_at_level(cells, depth - 1) > 0          # cells at the finest level exist
    cams = _cameras(corner, block)
    refs = [oracle.render(placed, cam, threads=8) for cam in cams]
    empty = host.Scene({**placed.blobs, 0: np.zeros(16, np.uint32)}, None, "empty")
    coarser = _with_ints(placed, max_depth=9) if depth == 10 else None
    for cam, ref in zip(cams, refs):
        assert _differ(ref, oracle.render(empty, cam, threads=8)) >= 0.2, "the tree is not in view"
        if coarser is not None:
            assert _differ(ref, oracle.render(coarser, cam, threads=8)) >= 0.05, "level 10 is not in front of the camera"
    return placed, cams, refs


def _row_id(row):
    form, depth, resident, full, brick = row
    return f"{'pow2' if form == POW2 else 'table'}-d{depth}-{'lds' if resident else 'mem'}" + ("-full" if full else "") + ("-brick" if brick else "")


def row_switches(row):
    """The environment switches that select the row where its tree alone would select a more specialised build."""
    form, depth, resident, full, brick = row
    names = []
    if form == POW2 and not resident and not brick:
        names.append("TDT_NO_BRICKS")
    if form == POW2 and resident and not full and depth in (5, 6):
        names.append("TDT_NO_FULL_GRID")
    return names


def test_the_rows_are_the_librarys_builds():
    """A build added to kTraceVariants without a scene here fails this test; it is not skipped."""
    mine = [row + (unit,) for row in ROWS for unit in (0, 1)]
    assert len(ROWS) == 33 and len(set(mine)) == 66
    theirs = rt.trace_variants()
    assert len(theirs) == len(set(theirs))
    assert set(mine) == set(theirs)


@pytest.mark.parametrize("unit", [1, 0], ids=["unit", "mul"])
@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_build_runs_and_equals_the_oracle(oracle, row, unit, monkeypatch):
    for name in row_switches(row):
        monkeypatch.setenv(name, "1")
    scene, cams, refs = _case(oracle, row, unit, ROWS.index(row))
    for name, cam, ref in zip(("inside", "outside"), cams, refs):
        r = rt.Renderer(scene, cam)
        try:
            first = r.render()
            v1 = r.ctx.last_variant()
            again = r.render()                                            # the cost-ordered replay
            v2 = r.ctx.last_variant()
        finally:
            r.close()
        for v in (v1, v2):
            assert (v["form"], v["depth"], v["resident"], v["full"], v["brick"], v["unit"]) == row + (unit,), name
        for frame, img in (("first", first), ("replay", again)):
            bad = (img.view(np.uint32) != ref.view(np.uint32)).any(axis=2)
            assert not bad.any(), f"{name} camera, {frame} frame: {int(bad.sum())} of {W * H} pixels differ from the oracle, first at (x, y) = {tuple(int(i) for i in np.argwhere(bad)[0][::-1])}"
