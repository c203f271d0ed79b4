"""The numpy model of screen-space selection (tests/select_model.py) without a GPU: its voxel arithmetic is host.pick_grid_voxel's
record by record, the voxels it gives for the oracle's first hits are the scene's (place 0) or empty (place 1) without exception,
and the overlay and extract models have the properties the header promises."""
import numpy as np
import pytest

import select_model as model
from octree_util import expand_cells
from tdt4230_project_raytracing_amd import host, rt

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- ids_from_hits against the host, record by record -------------------------------------------------------------------------
def _records(depth, mn, scale):
    """Synthetic hits around cell boundaries: on each axis in turn the point lies on plane k / 2^depth of the grid, k at both faces
    of the grid, next to them and in the middle, exactly and one and two float32 steps to either side; that axis' normal is -1, +1,
    +0 or -0 (the other two axes sit inside a cell with a zero normal).  With place 1 / place 0 the planes at the grid's faces
    give the cells just outside each face.  Then misses, iteration limits and stale records of the same geometry."""
    n = 1 << depth
    mn = np.asarray(mn, F)
    recs = []
    for axis in range(3):
        for k in sorted({0, 1, n // 2, n - 1, n}):
            plane = F(mn[axis] + F(scale) * F(k / n))
            for steps in (-2, -1, 0, 1, 2):
                p = plane
                for _ in range(abs(steps)):
                    p = np.nextafter(p, F(np.inf if steps > 0 else -np.inf))
                for normal in (F(-1.0), F(1.0), F(0.0), F(-0.0)):
                    r = np.zeros((), rt.RAY_HIT_DTYPE)
                    r["status"], r["fresh_record"], r["material"], r["t"] = rt.RAY_HIT, 1, 3, 0.5
                    r["point"] = mn + F(scale) * F((n // 3 + 0.37) / n)
                    r["point"][axis] = p
                    r["normal"][axis] = normal
                    recs.append(r)
    recs = np.array(recs)
    special = recs[: 24].copy()
    special["status"][:8] = rt.RAY_MISS
    special["status"][8:16] = rt.RAY_ITER_LIMIT
    special["fresh_record"][16:] = 0
    nan = recs[:3].copy()
    nan["point"][:, 1] = np.nan
    return np.concatenate([recs, special, nan])


@pytest.mark.parametrize("depth", [1, 8, 10])
@pytest.mark.parametrize("mn,scale", [((-0.5, -0.5, -1.0), 1.0), ((0.1, -0.3, 0.7), 0.75), ((-3.0, 2.0, 0.0), 3.0)])
def test_ids_from_hits_is_pick_grid_voxel(depth, mn, scale):
    floats = np.array([mn[0], mn[1], mn[2], 0.0, scale, 1.0 / scale, 1.0 / 64.0], F)
    ints = np.array([depth, 100, 64], np.int32)
    recs = _records(depth, mn, scale)
    seen = set()
    for place in (0, 1):
        ids = model.ids_from_hits(recs, floats, ints, place)
        assert (_bits(recs["t"]) == ids["t"]).all() and (ids["material"] == recs["material"]).all()
        for r, t in zip(recs, ids):
            try:
                v = host.pick_grid_voxel(r, (floats, ints), place)
            except ValueError:
                assert t["state"] == 0 and t["key"] == 0
                seen.add("refused")
                continue
            assert t["state"] == 1
            assert t["key"] == model.morton(v[0], v[1], v[2]) and (model.voxel_of(t["key"]) == v).all()
            seen.add(("valid", int(v.max()) == (1 << depth) - 1, int(v.min()) == 0))
    # both faces of the grid were reached from inside, and refusals happened (misses, stale records, cells outside each face)
    assert "refused" in seen and any(s != "refused" and s[1] for s in seen) and any(s != "refused" and s[2] for s in seen)


def test_cells_outside_each_face_are_refused():
    floats, ints = np.array([-0.5, -0.5, -1.0, 0.0, 1.0, 1.0, 1.0 / 64], F), np.array([8, 100, 64], np.int32)
    for axis in range(3):
        for face, normal in ((0, -1.0), (1, 1.0)):
            r = np.zeros(1, rt.RAY_HIT_DTYPE)
            r["status"], r["fresh_record"] = rt.RAY_HIT, 1
            r["point"] = floats[:3] + F(0.5)
            r["point"][0, axis] = floats[axis] + F(face)
            r["normal"][0, axis] = normal
            out_, in_ = model.ids_from_hits(r, floats, ints, 1)[0], model.ids_from_hits(r, floats, ints, 0)[0]
            assert out_["state"] == 0 and in_["state"] == 1
            assert model.voxel_of(in_["key"])[axis] == (255 if face else 0)
            with pytest.raises(ValueError):
                host.pick_grid_voxel(r, (floats, ints), 1)


# ---- the oracle's first hits --------------------------------------------------------------------------------------------------
W, H = 64, 48
# (origin, yaw, pitch, fov).  A pick is not always the voxel one sees: the traversal steps `adv` past a cell's face and pads empty
# cells by 1e-5 (a hundredth of a depth-10 voxel), so a grazing ray can enter a leaf through the corner of its neighbour, and the
# record of a hit found on iteration 0 is the root face's.  tdt_pick_grid_voxel then names a neighbour of the leaf that was hit, and
# the id image, which is that function per pixel, says the same.  On the demo scene's 1024^3 grid the poses tried first, those of
# tests/test_gpu_raycast.py, do this: ((0.0, 0.2, 0.9), 0, -8, 90) at 1 of 436 hits (a root-face record 0.003 voxels from a cell
# boundary), ((0.0, -0.1, -0.3), 0, 0, 90) at 3 of 1551 with place 0 and 95 with place 1.  They were replaced, with the oracle
# alone, by poses with no such pixel; nothing is tolerated.  config1's poses are the first tried.  Neither scene has a merged
# leaf in view (every leaf the demo's self-referencing cells reach lies on the finest level), so config2 supplies those.
CASES = {
    ("demo", "outside"): ((0.3, 0.4, 1.1), -12.0, -17.0, 60.0),
    ("demo", "inside"): ((0.16, 0.04, -0.39), 285.0, -40.0, 20.0),
    ("config1", "outside"): ((0.0, 0.2, 0.9), 0.0, -8.0, 90.0),
    ("config1", "inside"): ((0.0, -0.1, -0.3), 0.0, 0.0, 90.0),
    ("config2", "outside"): ((0.3, 0.4, 1.1), -12.0, -17.0, 60.0),
}
MERGED = {("config2", "outside")}                     # cases that must hit leaves above the finest level


def case_scene(name):
    return host.Scene.demo() if name == "demo" else host.Scene.config(int(name[-1]))


def _cam(origin, yaw, pitch, fov):
    c = host.Camera(fov, W, aspect_ratio=F(W) / F(H), origin=origin, viewport_height=2.0, samples_per_pixel=1, max_bounce=1)
    if yaw:
        c.turn_yaw(yaw)
    if pitch:
        c.turn_pitch(pitch)
    return c.uniforms()


def oracle_hits(oracle, scene, pose):
    """Records of rt.RAY_HIT_DTYPE (status, material, point, normal; fresh_record = 1) from the oracle's first-bounce carry of
    sample 0, as tests/test_denoise_model.py::oracle_guide reads it: every material Lambertian with an albedo of its own, so that
    the colour names the material or the sky; the record is the leaf call site's when that one is non-zero, else the root's."""
    n_mat = len(scene.blobs[1]) // 3
    mats = np.zeros((n_mat, 3), np.uint32)
    mats[:, 2] = np.arange(n_mat)
    i = np.arange(n_mat, dtype=F)
    alb = np.stack([(i + 1) / F(n_mat + 2), F(1) - (i + 1) / F(n_mat + 3), np.full(n_mat, 0.25, F)], 1).astype(F)
    blobs = dict(scene.blobs)
    blobs[1], blobs[2] = mats.reshape(-1), alb.reshape(-1)
    accum, carry = np.zeros((H, W, 4), F), np.zeros((H, W, 16), F)
    oracle.accumulate(host.Scene(blobs, name=scene.name + "_lamb"), _cam(*pose), accum, carry, 0, 1, dispatch=(W, 2 * H), threads=8)
    hit = _bits(accum[..., 2]) == _bits(F(0.25))
    leaf = (carry[..., 8:11] != 0).any(-1)
    out = np.zeros((H, W), rt.RAY_HIT_DTYPE)
    out["status"] = np.where(hit, rt.RAY_HIT, rt.RAY_MISS)
    out["fresh_record"] = 1
    out["material"] = np.where(hit, np.argmin(np.abs(accum[..., 0:1] - alb[None, None, :, 0]), -1), 0)
    out["normal"] = np.where(leaf[..., None], carry[..., 8:11], carry[..., 0:3])
    out["point"] = np.where(leaf[..., None], carry[..., 12:15], carry[..., 4:7])
    return out


def tree_lookup(cells, depth, xyz):
    """(occupied, level of the node that decides) for (n, 3) grid voxels: the logical tree as treeLookup resolves it."""
    cells = np.asarray(cells, np.uint32).reshape(-1, 8, 2)
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    cell = np.zeros(len(xyz), np.int64)
    occ, level_of, live = np.zeros(len(xyz), bool), np.zeros(len(xyz), np.int64), np.ones(len(xyz), bool)
    for level in range(1, depth + 1):
        b = (xyz >> (depth - level)) & 1
        node = cells[np.minimum(cell, len(cells) - 1), b[:, 0] * 4 + b[:, 1] * 2 + b[:, 2]]
        typ = np.where(cell < len(cells), node[:, 1], 0)
        leaf, parent = live & (typ == 2), live & (typ == 1) & (level < depth)
        occ |= leaf
        level_of[live & ~parent] = level
        live = parent
        cell = np.where(parent, node[:, 0].astype(np.int64), 0)
    return occ, level_of


def test_tree_lookup_is_expand_cells():
    scene = host.Scene.config(1)
    depth = scene.max_depth
    vox = expand_cells(scene.blobs[0], depth)
    n = 1 << depth
    grid = np.stack(np.meshgrid(*([np.arange(n)] * 3), indexing="ij"), -1).reshape(-1, 3)
    occ, _ = tree_lookup(scene.blobs[0], depth, grid)
    want = np.zeros((n, n, n), bool)
    want[vox[:, 0], vox[:, 1], vox[:, 2]] = True
    assert (occ.reshape(n, n, n) == want).all() and occ.sum() == len(vox)


@pytest.mark.parametrize("name,pose", sorted(CASES))
def test_the_voxel_of_every_first_hit_is_in_the_scene_or_just_outside_it(oracle, name, pose):
    """place 0: the voxel is one of the scene's (octree_util.expand_cells where the scene is small enough to expand: the demo's
    2^28 voxels are looked up in the tree instead); place 1: it is not.  No exceptions: the share must be 0."""
    scene = case_scene(name)
    depth = scene.max_depth
    hits = oracle_hits(oracle, scene, CASES[name, pose])
    assert (hits["status"] == rt.RAY_HIT).sum() > 40
    voxel_keys = None
    if name != "demo":
        vox = expand_cells(scene.blobs[0], depth)
        voxel_keys = model.morton(vox[:, 0], vox[:, 1], vox[:, 2])
    for place in (0, 1):
        ids = model.ids_from_hits(hits, scene.blobs[6], scene.blobs[7], place)
        valid = ids["state"] == 1
        assert valid.sum() > 10
        occ, level = tree_lookup(scene.blobs[0], depth, model.voxel_of(ids["key"][valid]))
        if voxel_keys is not None:
            assert (np.isin(ids["key"][valid], voxel_keys) == occ).all()
        exceptions = int((~occ).sum()) if place == 0 else int(occ.sum())
        assert exceptions == 0, (name, pose, place, exceptions, int(valid.sum()))
        if place == 0 and (name, pose) in MERGED:         # hits on merged leaves: the deciding node lies above the finest level
            assert (level < depth).sum() > 10


# ---- overlay and extract ------------------------------------------------------------------------------------------------------
def _ids(rng, h, w, n_keys=6, p_state=0.8):
    """Random patches: blocks of 3x2 texels share a voxel drawn from a few, some texels have none."""
    keys = model.morton(*rng.integers(0, 1024, (3, n_keys)))
    pick = rng.integers(0, n_keys, ((h + 1) // 2, (w + 2) // 3))
    ids = np.zeros((h, w), model.ID_DTYPE)
    ids["key"] = keys[np.repeat(np.repeat(pick, 2, 0), 3, 1)[:h, :w]]
    ids["state"] = rng.random((h, w)) < p_state
    ids["key"][ids["state"] == 0] = 0
    ids["material"] = rng.integers(0, 5, (h, w))
    ids["t"] = rng.integers(0, 2 ** 31, (h, w))
    return ids, keys


def _style(fill=(1, .6, 0, .35), edge=(0, 1, 0, 1), edge_width=1, flags=0):
    return dict(fill=fill, edge=edge, edge_width=edge_width, flags=flags)


def _list(keys):
    v = model.voxel_of(np.asarray(keys, np.uint32))
    return np.concatenate([v, np.ones((len(v), 1), np.int32)], 1)


def test_overlay_model_properties():
    rng = np.random.default_rng(11)
    ids, keys = _ids(rng, 23, 37, p_state=0.97)
    img = rng.random((23, 37, 4)).astype(F)
    some = _list(keys[:3])
    # an empty list is the identity, and so is a list of voxels off the grid
    for empty in (np.zeros((0, 4), np.int32), np.array([[-1, 0, 0, 1], [0, 1024, 0, 1]], np.int32)):
        out, member, edge, counts = model.overlay(img, ids, empty, _style())
        assert _bits(out).tobytes() == _bits(img).tobytes() and counts == (23 * 37, int((ids["state"] == 1).sum()), 0, 0)
    # a = 0 keeps the colour's value (x * 1 + c * 0), a = 1 replaces it; alpha and non-members are untouched
    out, member, edge, _ = model.overlay(img, ids, some, _style(fill=(.2, .4, .6, 0.0), edge_width=0))
    assert member.any() and not member.all() and not edge.any() and (out == img).all()
    out, member, edge, _ = model.overlay(img, ids, some, _style(fill=(.2, .4, .6, 1.0), edge_width=0))
    assert (out[member][:, :3] == np.array([.2, .4, .6], F)).all() and (_bits(out[..., 3]) == _bits(img[..., 3])).all()
    assert _bits(out[~member]).tobytes() == _bits(img[~member]).tobytes()
    # edges of width 1 are the member pixels a 3x3 erosion removes (the image's border does not erode)
    out, member, edge, counts = model.overlay(img, ids, some, _style())
    padded = np.pad(member, 1, constant_values=True)
    eroded = np.ones_like(member)
    for dy in range(3):
        for dx in range(3):
            eroded &= padded[dy:dy + 23, dx:dx + 37]
    assert (edge == (member & ~eroded)).all() and edge.any() and (member & ~edge).any()
    assert counts[2] == member.sum() and counts[3] == edge.sum()
    assert (out[edge][:, :3] == np.array([0, 1, 0], F)).all()
    # order and duplicates of the list do not matter
    shuffled = np.concatenate([some[::-1], some, some[1:2]])
    assert _bits(model.overlay(img, ids, shuffled, _style())[0]).tobytes() == _bits(out).tobytes()
    # voxel edges are a superset of plain edges, and wider outlines of narrower ones
    for ew in (1, 2, 4):
        plain = model.overlay(img, ids, some, _style(edge_width=ew))[2]
        per_voxel = model.overlay(img, ids, some, _style(edge_width=ew, flags=model.VOXEL_EDGES))[2]
        assert (per_voxel | plain == per_voxel).all() and (ew > 1 or per_voxel.sum() > plain.sum())
        if ew > 1:
            assert (plain | model.overlay(img, ids, some, _style(edge_width=ew // 2))[2] == plain).all()


def test_extract_model_properties():
    rng = np.random.default_rng(12)
    ids, keys = _ids(rng, 19, 31)
    # the whole image: np.unique over the selected keys, the last texel in row-major order giving the material
    flat = ids.reshape(-1)
    flat = flat[flat["state"] == 1]
    uniq, first_rev = np.unique(flat["key"][::-1], return_index=True)
    want = np.concatenate([model.voxel_of(uniq), (flat["material"][::-1][first_rev] + 1)[:, None].astype(np.int32)], 1)
    got = model.extract_voxels(ids)
    assert (got == want).all() and (got == model.extract_voxels(ids, (-5, -5, 100, 100))).all()
    assert len({tuple(r) for r in flat[["key", "material"]].tolist()}) > len(uniq)          # some key carries two materials
    k = model.morton(got[:, 0], got[:, 1], got[:, 2])
    assert (np.diff(k.astype(np.int64)) > 0).all()
    # one pixel, an empty rectangle, a rectangle outside
    x, y = np.argwhere(ids["state"] == 1)[0][::-1]
    one = model.extract_voxels(ids, (x, y, x, y))
    assert len(one) == 1 and model.morton(*one[0, :3]) == ids["key"][y, x] and one[0, 3] == ids["material"][y, x] + 1
    assert len(model.extract_voxels(ids, (5, 5, 4, 9))) == 0 and len(model.extract_voxels(ids, (31, 0, 40, 5))) == 0
    bad = ids.copy()
    bad["material"][y, x] = 254
    with pytest.raises(ValueError):
        model.extract_voxels(bad)
    assert len(model.extract_voxels(bad, (x + 1, y + 1, 30, 18))) >= 0                       # (outside the rectangle it does not matter)
