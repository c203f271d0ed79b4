"""Axis-parallel rays lying in cell-face planes, through every way the library traces a ray, bit for bit.

A jittered pinhole camera never sends a ray whose direction has a component of exactly zero, nor one that starts exactly on a
cell face.  There the slab arithmetic leaves the ordinary: the reciprocal is +-inf, (corner - origin) * inf is 0 * inf = NaN for
the cells whose face the ray lies in, and a -0 component flips the infinity's sign.  Each build of the trace kernel has its own
hand-written treatment of those values (cube_slabs' inline v_max / v_max3 / v_min3 chain, hw_min / hw_max's choice of zero on a
(+0, -0) tie, q_rcp3's wave-wide IEEE branch, the unit builds' dropped + 0.0f, the brick / full-grid / LDS-table exit arithmetic,
the miss pre-pass, the stuck-ray cut).  The cameras of tests/degenerate_cams.py make every primary ray of a frame such a ray.

  a  the fixture frames (tests/golden/degenerate/, rendered by the reference shader itself; the CPU side is
     tests/test_oracle_degenerate.py): first frame and cost-ordered replay; the frames of cameras outside the octree, which go
     through the miss pre-pass, and the 16 spp frames again without it; one on a multi-device context
  b  every build of kTraceVariants by name (rows, trees, corners and switches of tests/test_gpu_build_matrix.py), three bundles each
  c  pick / raycast under the bundle cameras against the oracle's first hit, and hand-made rays along cell edges and diagonals
  d  progressive passes with carry

All comparisons are on the bits.  Every case first checks on the CPU, with the oracle alone, that it is what it claims
(degenerate_cams.premises): enough slab tests with a NaN operand, the tree in view, and a frame that changes when the camera
steps off the face."""
import numpy as np
import pytest

import degenerate_cams as dc
import test_gpu_build_matrix as bm
import test_gpu_raycast as rc
import test_oracle_degenerate as od
import tree_model
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu

F = np.float32
W, H = dc.W, dc.H


def _assert_frame(img, ref, what):
    bad = (img.view(np.uint32) != ref.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (x, y) = {tuple(int(i) for i in np.argwhere(bad)[0][::-1])}"


def _render_twice(scene, cam, **kw):
    r = rt.Renderer(scene, cam, **kw)
    try:
        first = r.render()
        v1 = r.ctx.last_variant()
        again = r.render()                                                # the cost-ordered replay
        v2 = r.ctx.last_variant()
    finally:
        r.close()
    return first, again, v1, v2


# ---- a: the reference's own frames ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", od.NAMES)
def test_fixture_frames(name, monkeypatch):
    golden, meta, scene, cam = od.load(name)
    first, again, _, _ = _render_twice(scene, cam)
    _assert_frame(first, golden, "first frame")
    _assert_frame(again, golden, "replay")
    if name == "config2_yplane":
        first, again, _, _ = _render_twice(scene, cam, devices=[0, 0, 0])
        _assert_frame(first, golden, "three shares of one device, first frame")
        _assert_frame(again, golden, "three shares of one device, replay")
    # The miss pre-pass runs before every frame of a camera outside the octree (dc.outside is the library's own rule; which fixtures
    # those are is pinned in tests/test_oracle_degenerate.py), so the frames above went through it: these do not.  The 16 spp frames
    # are rendered both ways wherever they stand.
    if dc.outside(scene, cam) or meta["spp"] >= 16:
        monkeypatch.setenv("TDT_NO_PREPASS", "1")
        first, again, _, _ = _render_twice(scene, cam)
        _assert_frame(first, golden, "without the pre-pass, first frame")
        _assert_frame(again, golden, "without the pre-pass, replay")


# ---- b: every build by name ----------------------------------------------------------------------------------------------
# The plane index k, on the row's finest grid, inside the detail block (whose edge is 2^source depth finest cells): the k of the
# fixtures, 2^(source depth) / 2 - 5, where the source scene has the cells for it.
def _k(source_depth):
    return {3: 3, 4: 5}.get(source_depth, (1 << source_depth) // 2 - 5)       # (the depth-4 terrain has no leaves above plane 3)


# A leaf whose own slab test misses hands back the zeroed record (raytracer.comp:426-433), and the ray scattered from it starts
# at the world origin.  Under the all-zero corner that point lies in the octree's min faces, so such a ray meets 0 * inf wherever
# the camera stands, and "no NaN once the camera steps off the face" cannot hold.  Config 5's tree produces such records under the
# x-in bundle: in these rows that bundle stands at ZERO_CORNERS[1] (min_y = -0) instead of the row's (0, 0, 0).
X_IN_CORNER = {"pow2-d9-mem": 1, "table-d10-mem": 1}


def _bundles(row, unit, index):
    """[(name, placed scene, camera, axis)] of one build: the three bundles in the row's detail block.
    y      a bundle in the face plane y = k, from the reference pose inside the block, looking along -z
    x-in   a bundle in the face plane x = k that starts outside, in front of the min z face, and looks along +z: every ray
           enters through that face (w_z == min_z) while lying in a face plane of the cells it meets
    y -0   the first with d_y = -0.  That needs origin.y = +0 (see degenerate_cams), so the plane y = k must be y = 0: the corner's
           y becomes -k / 2^depth.  The multiplying builds keep a zero component (min_x = +0), the unit builds have none."""
    form, depth, resident, full, brick = row
    scene, block = bm._scene(row)
    src_depth = bm._tree(depth, resident)[1].max_depth
    k = _k(src_depth)
    assert k % 2 == 1 and 0 < k < (1 << src_depth)
    b = F(block)
    corner = (bm.UNIT_CORNER if unit else bm.ZERO_CORNERS[index % 3]).astype(F)
    placed = tree_model.with_corner(scene, corner)
    out = []
    y = dc.face_coordinate(k, depth, 1.0, corner[1])
    out.append(("y", placed, dc.plane_bundle(1, (corner[0] + b * F(0.5), y, corner[2] + b * F(0.7))), 1))
    if not unit and bm._row_id(row) in X_IN_CORNER:
        assert not corner.any()
        corner = bm.ZERO_CORNERS[X_IN_CORNER[bm._row_id(row)]].astype(F)
        placed = tree_model.with_corner(scene, corner)
    x = dc.face_coordinate(k, depth, 1.0, corner[0])
    out.append(("x-in", placed, dc.plane_bundle(0, (x, corner[1] + b * F(0.4), corner[2] - b * F(0.05)), view=(0.0, 0.0, 1.0)), 0))
    c0 = np.array([bm.UNIT_CORNER[0] if unit else 0.0, -k / (1 << depth), corner[2]], F)
    assert (c0 != 0).all() == bool(unit) and dc.face_coordinate(k, depth, 1.0, c0[1]) == 0
    at_zero = tree_model.with_corner(scene, c0)
    out.append(("y -0", at_zero, dc.plane_bundle(1, (c0[0] + b * F(0.5), 0.0, c0[2] + b * F(0.7)), neg_zero=True), 1))
    for _, s, cam, axis in out:
        assert s.blobs[6][4] == 1.0 and s.blobs[6][5] == 1.0
        assert dc.axis_component_bits(cam, axis) == ([0x80000000] if dc.is_neg_zero(cam.horizontal[1]) else [0])
    return out


@pytest.mark.parametrize("unit", [1, 0], ids=["unit", "mul"])
@pytest.mark.parametrize("row", bm.ROWS, ids=bm._row_id)
def test_build_renders_the_bundles(oracle, row, unit, monkeypatch):
    for switch in bm.row_switches(row):
        monkeypatch.setenv(switch, "1")
    cases = []
    for name, scene, cam, axis in _bundles(row, unit, bm.ROWS.index(row)):
        try:                                                              # (every row meets the full premise: none falls back)
            ref, st, share = dc.premises(oracle, scene, cam, axis, "nan")
        except AssertionError as e:
            raise AssertionError(f"{name} bundle, premise: {e}") from None
        print(f"{bm._row_id(row)} {'unit' if unit else 'mul'} {name}: nan_slab_tests {st['nan_slab_tests']} view share {share:.3f}")
        cases.append((name, scene, cam, ref))
    for name, scene, cam, ref in cases:
        first, again, v1, v2 = _render_twice(scene, cam)
        for v in (v1, v2):
            assert (v["form"], v["depth"], v["resident"], v["full"], v["brick"], v["unit"]) == row + (unit,), name
        _assert_frame(first, ref, f"{name} bundle, first frame, against the oracle")
        _assert_frame(again, ref, f"{name} bundle, replay, against the oracle")


# ---- c: queries ------------------------------------------------------------------------------------------------------------
QW, QH = 64, 48
_XY = np.stack(np.meshgrid(np.arange(QW), np.arange(QH)), -1).reshape(-1, 2).astype(np.int32)       # row-major: y outer, x inner


# Every fixture but config2_yplane_spp16 and config2_yplane_outside_spp16, whose twelve camera floats are config2_yplane's and
# config2_yplane_outside's: a query sees the uniforms only, so they would repeat those two cases.
QUERY_CASES = [n for n in od.NAMES if not n.endswith("_spp16")]


def test_the_query_cases_leave_out_only_repeated_uniforms():
    assert len(QUERY_CASES) == len(od.NAMES) - 2 >= 14
    for n in set(od.NAMES) - set(QUERY_CASES):
        assert dc.camera_bits(dc.fixture_case(n)[1]).tolist() == dc.camera_bits(dc.fixture_case(n[:-len("_spp16")])[1]).tolist()
        assert dc.FIXTURES[n][:2] == dc.FIXTURES[n[:-len("_spp16")]][:2]


@pytest.mark.parametrize("name", QUERY_CASES)
def test_picks_under_the_bundles_are_the_reference_first_hit(oracle, name):
    base, cam0, axis, kind = dc.fixture_case(name)
    scene, alb = rc._lambertian(base)
    cam = dc.camera_from_bits(dc.camera_bits(cam0), QW, QH, 4, 1)         # the same uniforms over 64 x 48, 1 bounce
    # the fixture's view premises are its own (tests/test_oracle_degenerate.py): a one-bounce Lambertian frame shows albedos, which
    # do not move with the camera.  Here: the frame's primary rays meet the NaNs, and only on the face ("nan"); infinities and no
    # NaN ("inf"); "view" (the tiny component) claims only its direction's bits, checked below
    st = oracle.render(scene, cam, threads=8, want_stats=True)[1]
    assert st["inf_slab_tests"] > 0
    if kind == "nan":
        nan_off = oracle.render(scene, dc.moved(cam, axis), threads=8, want_stats=True)[1]["nan_slab_tests"]
        assert st["nan_slab_tests"] >= dc.NAN_TESTS and nan_off == 0, (st["nan_slab_tests"], nan_off)
    if kind == "inf":
        assert st["nan_slab_tests"] == 0, st["nan_slab_tests"]
    print(f"{name}: nan_slab_tests {st['nan_slab_tests']} inf_slab_tests {st['inf_slab_tests']}")
    want = 0x80000000 if "negzero" in name else 0
    r = rt.Renderer(scene, cam)
    try:
        seen = 0
        for s in (0, 2):
            hits, rays = r.pick(_XY, sample=s, return_rays=True)
            d_axis = rays[:, 3 + axis].view(np.uint32)
            if "denormal" in name:                                       # 2^-140 * v / |d|: a denormal, or +0 where v == 0
                assert (d_axis < 0x00800000).all() and (d_axis > 0).any()
            elif "tiny" in name:
                # 2^-120 * v / |d|: positive, below the reciprocal's fast window (2^-100).  |d| < 2 under this 90 degree view, so the
                # component is a normal number wherever v >= 2^-5: all but the two image rows nearest v == 0
                assert (d_axis < 0x0D800000).all()
                assert (d_axis >= 0x00800000).sum() >= QW * (QH - 2)
            else:
                assert (d_axis == want).all(), f"{int((d_axis != want).sum())} rays with another d[{axis}] than {want:#x}"
            assert (rays[:, axis].view(np.uint32) == np.float32(cam.origin[axis]).view(np.uint32)).all()
            assert r.ctx.raycast(rays).tobytes() == hits.tobytes()
            n_hit, n_leaf = rc._assert_first_hit(oracle, scene, alb, cam, hits, rays, s, QW, QH)
            seen += n_leaf
        assert seen > 0
    finally:
        r.close()


# hand-made rays: the octree placed so that the face planes x = 0 and y = 0 are plane 27 of 64 (finest-level faces only)
EDGE_CORNER = np.array([-dc.K6 / 64, -dc.K6 / 64, -1.0], F)
S3 = F(1.0) / np.sqrt(F(3.0))                 # normalize((1, 1, 1)) as the shader computes it: x * (1 / sqrt(3))


def _hand_rays():
    """[(origin, direction given to raycast, direction given to degenerate_cams.line)].  Coordinates are multiples of 2^-7, so
    origin + direction is exact.  Along -z and along (-0, 0, 1): origins on a face plane in x and in y (on a cell edge; every odd
    plane of the 64), and in z as well (a cell corner) or between two z planes; (-0, 0, 1) needs origin.x = +0, and also starts
    outside, below the min z face.  The exact diagonal: from cell corners, both ways."""
    odd = [dc.face_coordinate(k, 6, 1.0, EDGE_CORNER[0]) for k in range(1, 64, 2)]
    rays = []
    for x in odd[::2]:
        for y in odd:
            for z in (F(-0.046875), F(-0.0390625)):                      # plane 61 of 64, and half a cell above it
                rays.append(((x, y, z), (0.0, 0.0, -1.0), (0.0, 0.0, -1.0)))
    for y in odd:
        for z in (F(-0.953125), F(-0.9609375), F(-1.25)):
            rays.append(((F(0.0), y, z), (F(-0.0), 0.0, 1.0), (F(-0.0), 0.0, 1.0)))
    for k in (2, 5, 9, 14, 20, 27):
        o = tuple(dc.face_coordinate(k, 6, 1.0, c) for c in EDGE_CORNER)
        rays.append((o, (S3, S3, S3), (1.0, 1.0, 1.0)))
        rays.append(((o[0], o[1], F(o[2] + F(0.5))), (-S3, -S3, -S3), (-1.0, -1.0, -1.0)))
    return rays


def test_hand_made_rays_along_edges_and_diagonals(oracle):
    """raycast of rays written down by hand against the oracle's first hit under a line camera that sends the same ray; the ray
    that camera's pick reports must be the hand-made one bit for bit, and its pick must be raycast's bytes."""
    base = tree_model.with_corner(host.Scene.config(2), EDGE_CORNER)
    scene, alb = rc._lambertian(base)
    # of the candidates: every ray that meets a NaN slab test (the oracle says which), and every eighth of the others
    hand, n_nan = [], 0
    for i, (o, d, d_cam) in enumerate(_hand_rays()):
        cam = dc.line(o, d_cam, w=2, h=2, spp=1, bounce=1)
        nan = oracle.render(scene, cam, threads=1, want_stats=True)[1]["nan_slab_tests"] > 0
        if nan or i % 8 == 0 or d[0] != 0:                               # (d[0] != 0: the diagonals)
            hand.append((o, d, cam))
            n_nan += nan
    assert n_nan >= 100 and len(hand) - n_nan >= 50, (n_nan, len(hand))
    rays = np.array([list(o) + list(d) for o, d, _ in hand], F)
    cams = [cam for _, _, cam in hand]
    xy = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.int32)
    r = rt.Renderer(scene, cams[0])
    try:
        hits = r.ctx.raycast(rays)
        n_hit = n_leaf = 0
        for i, cam in enumerate(cams):
            rt.initial_uniforms(cam, r.shader.program)
            picked, prays = r.pick(xy, sample=0, return_rays=True)
            assert (prays.view(np.uint32) == rays[i].view(np.uint32)[None, :]).all(), f"ray {i}: the line camera sends {prays[0].tolist()}"
            assert all(picked[j:j + 1].tobytes() == hits[i:i + 1].tobytes() for j in range(4)), f"ray {i}: pick and raycast differ"
            got, leaf = rc._assert_first_hit(oracle, scene, alb, cam, picked, prays, 0, 2, 2)
            n_hit += got > 0
            n_leaf += leaf > 0
    finally:
        r.close()
    assert n_leaf >= 100, (n_hit, n_leaf, len(hand))


# ---- d: progressive ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-device", "two-shares"])
def test_progressive_passes_on_the_bundle(oracle, devices):
    import torch
    golden, meta, scene, cam = od.load("config2_yplane_spp16")
    spp = cam.samples_per_pixel
    ref = oracle.render(scene, cam, threads=8)
    _assert_frame(ref, golden, "the oracle against the reference's frame")
    dw, dh = W + 1, H + 1
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    carry = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r = rt.Renderer(scene, cam, devices=devices) if devices else rt.Renderer(scene, cam, image_ptr=accum.data_ptr())
    try:
        for begin, count in ((0, 5), (5, 3), (8, 8)):
            r.shader.dispatch_accumulate(dw, dh, 1, begin, count, 1 if devices else carry.data_ptr())
        r.shader.dispatch_resolve(dw, dh, 1, spp)
        img = r.texture.read()
        _assert_frame(img, ref, "three passes and a resolve")
        if devices:
            _assert_frame(r.render(), ref, "the one-pass frame afterwards")
    finally:
        r.close()
    one, again, _, _ = _render_twice(scene, cam)
    _assert_frame(one, ref, "one pass")
    _assert_frame(img, one, "three passes against one pass")
