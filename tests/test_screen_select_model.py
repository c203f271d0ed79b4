"""The numpy model of through-selection (tests/screen_select_model.py) without a GPU: its projection is reproject_model's bit for
bit, the three shapes agree where the header says they are one, the polygon rule is a brute-force point-in-polygon's, the window
marquee and the filters only remove voxels, and the committed cases (tests/screen_select_cases.py) reach every outcome the kernel
can take."""
from fractions import Fraction

import numpy as np
import pytest

import reproject_model
import screen_select_cases as cases
import screen_select_model as model

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _run(tree, floats, cam, W, H, shape, seed=0, **kw):
    depth, V = cases.trees()[tree]
    fl = cases.FLOATS[floats]
    view = cases.cameras(V, depth, fl, W, H)[cam]
    sel_kw, polygon, mask = cases.shapes(W, H, seed)[shape]
    sel = model.sel_of(**sel_kw, **kw)
    return model.extract(V, fl, cases.ints_of(depth), view, sel, polygon, mask)


# ---- Q ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", sorted(cases.FLOATS))
@pytest.mark.parametrize("cam", ["outside", "inside", "centre"])
def test_q_is_reproject_models_bits(floats, cam):
    """The same world points as the hit points of a reprojection (origin 0, direction w, t = 1): Q, the on-screen test and the
    counts are reproject_model.reproject's."""
    depth, V = cases.trees()["n2048"]
    fl = cases.FLOATS[floats]
    W, H = 64, 48
    view = cases.cameras(V, depth, fl, W, H)[cam]
    w = model.world_points(2 * V[:, :3].astype(np.int64) + 1, depth, fl)
    n = len(w)
    rays = np.zeros((1, n, 6), F)
    rays[0, :, 3:] = w
    guide = np.zeros((1, n), [("kind", "<u4"), ("material", "<u4"), ("plane", "<f4"), ("t", "<f4")])
    guide["kind"], guide["t"] = 1, 1.0
    prev_guide = np.zeros((H, W), guide.dtype)
    prev_guide["kind"] = 1
    prev_hist = np.ones((H, W, 4), F)
    _, _, Q, found, counts = reproject_model.reproject(rays, guide, np.zeros((1, n, 4), F), 1, view, prev_guide, prev_hist, 64.0)
    on, px, py, _ = model.project(w, view)
    assert np.array_equal(found[0], on) and counts[1] == int(on.sum()) and counts[3] == n - int(on.sum())
    assert np.array_equal(Q[0, :, 0], px) and np.array_equal(Q[0, :, 1], py)
    assert 0 < on.sum() < n


def test_world_points_round_twice_and_never_fuse():
    """Every doubled coordinate of a depth-10 grid: the product is rounded before the add.  The cases tell the two apart: a fused
    multiply-add (one rounding, computed here in float64, which holds the product exactly) gives other bits for some of them."""
    fl = cases.FLOATS["odd"]
    k2 = np.repeat(np.arange(2049, dtype=np.int64)[:, None], 3, 1)
    w = model.world_points(k2, 10, fl)
    u = k2 / 2048.0
    want = ((u.astype(F) * fl[4]).astype(F) + fl[:3]).astype(F)
    fused = (u * np.float64(fl[4]) + fl[:3].astype(np.float64)).astype(F)
    assert np.array_equal(_bits(w), _bits(want))
    assert (_bits(w) != _bits(fused)).any()


# ---- the shapes agree ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree,floats,cam,size", [("n2048", "unit", "outside", (64, 48)), ("d10", "odd", "inside", (33, 17)),
                                                  ("n257", "odd", "outside", (33, 17)), ("n65", "unit", "inside", (2, 2))])
@pytest.mark.parametrize("window", [False, True])
def test_rect_polygon_and_mask_of_one_rectangle_select_the_same(tree, floats, cam, size, window):
    W, H = size
    rect, rc = _run(tree, floats, cam, W, H, "rect-part", window=window)
    poly, pc = _run(tree, floats, cam, W, H, "poly-rect", window=window)
    mask, mc = _run(tree, floats, cam, W, H, "mask-rect", window=window)
    assert rect.tobytes() == poly.tobytes() == mask.tobytes() and rc == pc == mc
    if size != (2, 2):
        assert 0 < rc[3] < rc[1] or window


def test_polygon_start_and_orientation_do_not_matter():
    W, H = 64, 48
    for name in ("poly-triangle", "poly-bowtie", "poly-circle", "poly-outside"):
        _, polygon, _ = cases.shapes(W, H)[name]
        polygon = model.check_polygon(polygon)
        base = model._polygon_table(polygon, W, H)
        assert base.any() and not base.all(), name
        for shift in (1, len(polygon) // 2):
            turned = polygon[shift:] + polygon[:shift]
            assert np.array_equal(model._polygon_table(turned, W, H), base), name
            assert np.array_equal(model._polygon_table(turned[::-1], W, H), base), name


def test_bow_tie_follows_even_odd():
    """(0,0) (W,H) (W,0) (0,H): the left and right triangles between the diagonals are inside, the top and bottom ones are not."""
    W, H = 64, 48
    t = model._polygon_table(model.check_polygon(cases.shapes(W, H)["poly-bowtie"][1]), W, H)
    assert t[H // 2, 2] and t[H // 2, W - 3] and not t[2, W // 2] and not t[H - 3, W // 2]
    # a doubly wound square: the inner square is wound twice, which even-odd calls outside
    twice = model.check_polygon([(0, 0), (40, 0), (40, 40), (0, 40), (0, 0), (40, 0), (40, 40), (0, 40)])
    assert not model._polygon_table(twice, W, H).any()


def test_table_is_the_pixel_rule_and_lies_in_the_bounding_box():
    """The row-wise table equals pixel_in_polygon, and a pixel inside has xmin <= px < xmax and ymin <= py < ymax of the vertices: the
    bounding-box rejection of the kernel removes nothing."""
    W, H = 33, 17
    rng = np.random.default_rng(5)
    for name, (_, polygon, _) in cases.shapes(W, H).items():
        if polygon is None:
            continue
        polygon = model.check_polygon(polygon)
        t = model._polygon_table(polygon, W, H)
        for px, py in rng.integers(0, [W, H], size=(60, 2)):
            assert t[py, px] == model.pixel_in_polygon(px, py, polygon), (name, px, py)
        xs, ys = [p[0] for p in polygon], [p[1] for p in polygon]
        py, px = np.nonzero(t)
        assert (px >= min(xs)).all() and (px < max(xs)).all() and (py >= min(ys)).all() and (py < max(ys)).all(), name


def _brute_force(px, py, polygon):
    """Crossing number at the pixel centre with exact rationals; None when the centre lies on an edge."""
    x, y = Fraction(2 * px + 1, 2), Fraction(2 * py + 1, 2)
    n, count = len(polygon), 0
    for j in range(n):
        (ax, ay), (bx, by) = polygon[j], polygon[(j + 1) % n]
        if (ax, ay) == (bx, by):
            continue
        cross = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
        if cross == 0 and min(ax, bx) <= x <= max(ax, bx) and min(ay, by) <= y <= max(ay, by):
            return None
        if (ay > y) != (by > y):
            xc = ax + Fraction(bx - ax) * (y - ay) / (by - ay)
            if xc > x:
                count += 1
    return count % 2 == 1


def test_polygon_rule_against_a_brute_force_point_in_polygon():
    W, H = 40, 30
    rng = np.random.default_rng(2024)
    tested = excluded = 0
    for trial in range(40):
        n = int(rng.integers(3, 12))
        polygon = model.check_polygon(rng.integers(-10, [W + 10, H + 10], size=(n, 2)).tolist())
        t = model._polygon_table(polygon, W, H)
        for px, py in rng.integers(0, [W, H], size=(120, 2)):
            want = _brute_force(int(px), int(py), polygon)
            tested += 1
            if want is None:
                excluded += 1
                continue
            assert t[py, px] == want, (trial, px, py, polygon)
    assert tested == 4800 and excluded < 0.01 * tested, (tested, excluded)


# ---- window, filters -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree,floats,cam", [("n2048", "unit", "outside"), ("n257", "odd", "inside"), ("d10", "unit", "outside")])
def test_window_selects_a_subset_of_the_centre_rule_for_a_rectangle(tree, floats, cam):
    """A rectangle of pixels is convex and Q maps a voxel in front of the eye to a convex quadrilateral around its centre's image; the
    pixel grid's floor keeps the order on each axis.  (For a lasso or a mask no such inclusion holds.)"""
    W, H = 64, 48
    for shape in ("rect-part", "rect-all", "rect-clipped"):
        centre, cc = _run(tree, floats, cam, W, H, shape)
        window, wc = _run(tree, floats, cam, W, H, shape, window=True)
        keys = set(map(tuple, centre[:, :3]))
        assert all(tuple(v) in keys for v in window[:, :3]), shape
        assert wc[3] <= cc[3] and wc[0] == cc[0]


def test_filters_only_remove_voxels():
    W, H = 64, 48
    depth, V = cases.trees()["n2048"]
    m = int(V[len(V) // 3, 3]) - 1
    for shape in ("rect-all", "poly-circle", "mask-random"):
        for window in (False, True):
            base, bc = _run("n2048", "odd", "outside", W, H, shape, window=window)
            keys = set(map(tuple, base))
            for kw in (dict(material=m), dict(material=0), dict(min_distance=2.9), dict(max_distance=2.9), dict(min_distance=2.5, max_distance=3.2)):
                got, gc = _run("n2048", "odd", "outside", W, H, shape, window=window, **kw)
                assert all(tuple(v) in keys for v in got) and gc[:3] == bc[:3] and gc[3] <= bc[3], (shape, window, kw)
                if "material" in kw:
                    assert (got[:, 3] == kw["material"] + 1).all()
            # a range cuts the set in two: dd <= 2.9^2 and dd >= 2.9^2 overlap only in voxels at exactly that squared distance
            near, _ = _run("n2048", "odd", "outside", W, H, shape, window=window, max_distance=2.9)
            far, _ = _run("n2048", "odd", "outside", W, H, shape, window=window, min_distance=2.9)
            both = set(map(tuple, near)) & set(map(tuple, far))
            assert len(near) + len(far) - len(both) == len(base) and len(both) <= 1 and 0 < len(near) < len(base), (shape, window)


def test_edit_is_the_region_models_paint_and_clear():
    W, H = 33, 17
    depth, V = cases.trees()["n257"]
    fl = cases.FLOATS["unit"]
    view = cases.cameras(V, depth, fl, W, H)["outside"]
    sel = model.sel_of(model.RECT, rect=(5, 3, 25, 12))
    picked, counts = model.extract(V, fl, cases.ints_of(depth), view, sel)
    assert 0 < len(picked) < len(V)
    cleared, c2 = model.edit(V, fl, cases.ints_of(depth), view, sel, None, None, model.REGION_CLEAR)
    painted, c3 = model.edit(V, fl, cases.ints_of(depth), view, sel, None, None, model.REGION_PAINT, 200)
    assert c2 == c3 == counts and len(cleared) == len(V) - len(picked) and len(painted) == len(V)
    gone = set(map(tuple, picked[:, :3]))
    assert not any(tuple(v) in gone for v in cleared[:, :3])
    assert (painted[[tuple(v) in gone for v in painted[:, :3]], 3] == 201).all() and (painted[:, 3] == 201).sum() >= len(picked)


# ---- the committed cases reach every outcome ------------------------------------------------------------------------------------------
def test_cases_reach_every_outcome():
    W, H = 64, 48
    for tree in ("n2048", "d10", "n257"):
        depth, V = cases.trees()[tree]
        for floats in sorted(cases.FLOATS):
            fl = cases.FLOATS[floats]
            views = cases.cameras(V, depth, fl, W, H)
            k = V[:, :3].astype(np.int64)
            centres = model.world_points(2 * k + 1, depth, fl)
            # voxels behind a camera inside the grid, and voxels in front of it but off screen
            ru, rv, rw, _ = reproject_model.view_rows(views["inside"])
            nw = reproject_model._dot(rw, (centres - views["inside"]["origin"]).astype(F))
            on, _, _, _ = model.project(centres, views["inside"])
            assert (nw < 0).sum() > 0 and ((nw > 0) & ~on).sum() > 0 and on.sum() > 0, (tree, floats)
            on, _, _, _ = model.project(centres, views["outside"])
            assert 0 < on.sum() < len(V), (tree, floats)
            # the voxel whose centre is the eye: nw = 0, and it fails
            d = (centres - views["centre"]["origin"]).astype(F)
            at_eye = (d == 0).all(1)
            on, _, _, _ = model.project(centres, views["centre"])
            assert at_eye.sum() == 1 and not on[at_eye][0], (tree, floats)
            all_c, counts = _run(tree, floats, "centre", W, H, "rect-all")
            assert counts[1] == counts[2] == counts[3] == int(on.sum()) < counts[0] == len(V)
            # a voxel straddling the image edge under WINDOW: its centre is on screen, one of its corners is not
            cam = "outside" if tree != "d10" else "inside"
            centre, cc = _run(tree, floats, cam, W, H, "rect-all")
            window, wc = _run(tree, floats, cam, W, H, "rect-all", window=True)
            assert wc[1] < cc[1] and wc[1] == wc[2] == wc[3] == len(window), (tree, floats)


def test_every_shape_selects_something_and_not_everything_somewhere():
    seen = {}
    for (W, H) in cases.IMAGES:
        for shape in cases.shapes(W, H):
            for window in (False, True):
                got, counts = _run("n2048", "unit", "outside", W, H, shape, window=window)
                seen.setdefault((shape, window), []).append(counts)
    for (shape, window), cs in seen.items():
        if shape == "rect-empty":
            assert all(c[2] == 0 for c in cs)
        else:
            assert any(0 < c[2] < c[0] for c in cs) or (window and shape == "rect-pixel"), (shape, window, cs)


def test_model_refuses_what_the_call_refuses():
    with pytest.raises(AssertionError):
        model.check_polygon([(0, 0), (1, 1)])
    with pytest.raises(AssertionError):
        model.check_polygon([(0, 0), (1, 1), (0, (1 << 20) + 1)])
    model.check_polygon([(0, 0), (-(1 << 20), 1), (0, 1 << 20)])
    with pytest.raises(AssertionError):
        model.check_polygon([(i, i * i) for i in range(257)])
