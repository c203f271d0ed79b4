"""The whole-depth table's entries that carry the cell corner (csrc/tdt_rt.hip build_full_grid_kernel, csrc/trace_device.hpp
full_entry_decode): the exhaustive device check of every table position (tdt_selftest 17), and renders of trees made for the
table against the oracle, bit for bit.

Trees.  One per depth (5 and 6), from a voxel list through the numpy builder of tests/tree_model.py.  Two chains of nested blocks
run from the root into the grid's two opposite corners: at every level l the chain's block has one child filled with one material
(a LEAF at level l), six children empty (EMPTY at level l) and one child that carries the chain on, down to the single voxels
(0, 0, 0) and (2^D - 1,) * 3 — finest-level cells whose corner digits are 0 and 2^D - 1.  Level 1 has a filled octant and an
empty one beside the two chain octants; the three octants left hold random single voxels, which make finest-level cells all
over.  The decode depends on the tree and not on the image, so the images are small."""
import numpy as np
import pytest

import tree_cases
import tree_model
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

EMPTY, PARENT, LEAF = 0, 1, 2
POW2 = 1
SPP, BOUNCE = 4, 4
N_MATERIALS = 20                              # of config 2, whose material tables the scenes borrow

_trees, _scenes, _refs = {}, {}, {}


def _voxels(depth):
    g, h = 1 << depth, 1 << (depth - 1)
    rng = np.random.default_rng(1700 + depth)
    out = [tree_cases.cube((0, h, 0), h, 3)]                              # octant (0, 1, 0): a LEAF at level 1; octant (1, 0, 0): EMPTY
    for l in range(2, depth + 1):
        s = 1 << (depth - l)                                             # side of a level-l block
        out.append(tree_cases.cube((s, s, s), s, 1 + l % N_MATERIALS))    # near chain: child 7 of the chain's block is a LEAF, child 0 goes on
        out.append(tree_cases.cube((g - 2 * s,) * 3, s, 8 + l))           # far chain: child 0 is a LEAF, child 7 goes on
    out.append(np.array([[0, 0, 0, 5], [g - 1, g - 1, g - 1, 6]], np.int64))
    for ox, oy, oz in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        idx = rng.permutation(h ** 3)[: 40 * depth]
        p = np.stack([idx // (h * h), (idx // h) % h, idx % h], 1) + np.array([ox, oy, oz]) * h
        out.append(np.concatenate([p, rng.integers(1, N_MATERIALS + 1, size=(len(p), 1))], 1))
    return np.concatenate(out).astype(np.int32)


def _levels(cells, depth):
    """{level: set of node types met at that level} by walking the PARENTs down from cell 0, and the finest-level digits met."""
    c = np.asarray(cells, np.uint32).reshape(-1, 8, 2)
    child = np.array([[k >> 2, (k >> 1) & 1, k & 1] for k in range(8)], np.int64)
    cell, base, kinds, digits = np.zeros(1, np.int64), np.zeros((1, 3), np.int64), {}, set()
    for level in range(1, depth + 1):
        nodes = c[cell]
        pos = base[:, None, :] * 2 + child[None, :, :]
        kinds[level] = set(np.unique(nodes[..., 1]).tolist())
        if level == depth:
            digits = set(np.unique(pos[nodes[..., 1] == LEAF]).tolist())
        par = nodes[..., 1] == PARENT
        cell, base = nodes[..., 0][par].astype(np.int64), pos[par]
    return kinds, digits


def _tree(depth):
    if depth not in _trees:
        cells = tree_model.build_cells(_voxels(depth), depth)
        kinds, digits = _levels(cells, depth)
        for level in range(1, depth + 1):
            assert {EMPTY, LEAF} <= kinds[level], f"level {level} lacks an EMPTY or a LEAF"
        assert {0, (1 << depth) - 1} <= digits
        assert cells.size // 16 <= 5120                                  # inside the LDS table
        cells.setflags(write=False)
        _trees[depth] = cells
    return _trees[depth]


def _scene(depth, cells=None, materials=None):
    key = depth if cells is None else None
    if key is not None and key in _scenes:
        return _scenes[key]
    like = host.Scene.config(2)
    scene = tree_model.scene_from_cells(_tree(depth) if cells is None else cells, depth, 1 << 16, like)
    if materials is not None:
        scene.blobs[1] = materials
    if key is not None:
        _scenes[key] = scene
    return scene


def _camera(w, h, pose):
    if pose == "reference":
        return host.camera_reference_pose(w, h, SPP, BOUNCE)
    # the reference pose's eye (main.rs:165-168: (0.5, 0.4, 0.7) from the corner (-0.5, -0.5, -1)), turned to look along +x
    f32 = np.float32
    o, d, right, up = np.array([0.0, -0.1, -0.3], f32), np.array([1, 0, 0], f32), np.array([0, 0, 1], f32), np.array([0, 1, 0], f32)
    vh = f32(2.0)
    hor, ver = right * (f32(w) / f32(h) * vh), up * vh
    llc = o - hor * f32(0.5) - ver * f32(0.5) + d
    u = host.CameraUniforms()
    u.image_width, u.image_height, u.samples_per_pixel, u.max_bounce = w, h, SPP, BOUNCE
    for name, v in (("horizontal", hor), ("vertical", ver), ("lower_left_corner", llc), ("origin", o)):
        getattr(u, name)[:] = [float(x) for x in v.astype(f32)]
    return u


def _same(img, ref, what):
    bad = (img.view(np.uint32) != ref.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ from the oracle, first at (x, y) = {tuple(int(i) for i in np.argwhere(bad)[0][::-1])}"


def _full(v):
    return (v["form"], v["depth"], v["resident"], v["full"], v["brick"])


def _node_of(cells, depth, p):
    """Index of the node the descent to voxel p ends on."""
    v = 0
    for level in range(1, depth + 1):
        sh = depth - level
        idx = ((2 * v + ((p[0] >> sh) & 1)) << 2) + (((p[1] >> sh) & 1) << 1) + ((p[2] >> sh) & 1)
        if cells[2 * idx + 1] != PARENT:
            return idx, level
        v = int(cells[2 * idx])
    raise AssertionError("a PARENT at the finest level")


@pytest.mark.parametrize("depth", [5, 6])
def test_every_table_position_decodes_as_the_16_bit_entry_and_the_walk(depth):
    scene = _scene(depth)
    r = rt.Renderer(scene, _camera(2, 2, "reference"))
    try:
        assert r.ctx.selftest(17) == 0
    finally:
        r.close()


@pytest.mark.parametrize("pose", ["reference", "plus_x"])
@pytest.mark.parametrize("size", [33, 2])
@pytest.mark.parametrize("depth", [5, 6])
def test_render_equals_the_oracle(oracle, depth, size, pose):
    scene, cam = _scene(depth), _camera(size, size, pose)
    ref = oracle.render(scene, cam, threads=4)
    if size == 33:
        empty = host.Scene({**scene.blobs, 0: np.zeros(16, np.uint32)}, None, "empty")
        assert (ref.view(np.uint32) != oracle.render(empty, cam, threads=4).view(np.uint32)).any(axis=2).mean() >= 0.1, "the tree is not in view"
    r = rt.Renderer(scene, cam)
    try:
        first = r.render()
        v1 = r.ctx.last_variant()
        again = r.render()
        v2 = r.ctx.last_variant()
    finally:
        r.close()
    assert _full(v1) == (POW2, depth, 1, 1, 0) and _full(v2) == (POW2, depth, 1, 1, 0)
    _same(first, ref, "first frame")
    _same(again, ref, "replay")


@pytest.mark.parametrize("index,full", [(2047, 1), (2048, 0)])
def test_material_index_limit(oracle, index, full):
    """A LEAF whose material index is the largest the entry's 11 bits hold runs the whole-depth build; one more falls back."""
    depth = 6
    cells = _tree(depth).copy()
    h = 1 << (depth - 2)
    node, level = _node_of(cells, depth, (h, h, h))                       # the level-2 LEAF of the near chain: in view of the reference pose
    assert level == 2 and cells[2 * node + 1] == LEAF
    cells[2 * node] = index
    like = host.Scene.config(2).blobs[1].reshape(-1, 3)
    materials = np.ascontiguousarray(np.tile(like, (103, 1))[:2049].reshape(-1))      # a real material behind every index up to 2048
    scene = _scene(depth, cells, materials)
    cam = _camera(33, 33, "reference")
    ref = oracle.render(scene, cam, threads=4)
    r = rt.Renderer(scene, cam)
    try:
        img = r.render()
        v = r.ctx.last_variant()
    finally:
        r.close()
    assert (v["form"], v["depth"], v["resident"], v["full"]) == (POW2, depth, 1, full)
    _same(img, ref, f"material index {index}")


def test_table_is_rebuilt_after_an_edit(oracle):
    """tdt_buffer_sub_data turns one finest-level LEAF that the camera sees into EMPTY between two frames."""
    depth = 6
    scene, cam = _scene(depth), _camera(33, 33, "reference")
    before = oracle.render(scene, cam, threads=4)
    vox = _voxels(depth)
    h = 1 << (depth - 1)
    loose = vox[(vox[:, 0] >= h) & (vox[:, 1] >= h) & (vox[:, 2] < h)][:, :3]          # octant (1, 1, 0): in front of the camera
    for q in loose[:60]:
        node, level = _node_of(scene.blobs[0], depth, q)
        if level != depth or scene.blobs[0][2 * node + 1] != LEAF:
            continue
        cells = scene.blobs[0].copy()
        cells[2 * node: 2 * node + 2] = 0
        edited = _scene(depth, cells)
        after = oracle.render(edited, cam, threads=4)
        if (after.view(np.uint32) != before.view(np.uint32)).any():
            break
    else:
        raise AssertionError("no finest-level LEAF in view")
    r = rt.Renderer(scene, cam)
    try:
        _same(r.render(), before, "before the edit")
        r.vbos[0].sub_data(8 * node, np.zeros(2, np.uint32))
        img = r.render()
        v = r.ctx.last_variant()
        assert r.ctx.selftest(17) == 0
    finally:
        r.close()
    assert _full(v) == (POW2, depth, 1, 1, 0)
    _same(img, after, "after the edit")


def test_table_off(oracle, monkeypatch):
    monkeypatch.setenv("TDT_NO_FULL_GRID", "1")
    depth = 6
    scene, cam = _scene(depth), _camera(33, 33, "reference")
    ref = oracle.render(scene, cam, threads=4)
    r = rt.Renderer(scene, cam)
    try:
        img = r.render()
        v = r.ctx.last_variant()
    finally:
        r.close()
    assert _full(v) == (POW2, depth, 1, 0, 0)
    _same(img, ref, "TDT_NO_FULL_GRID=1")
