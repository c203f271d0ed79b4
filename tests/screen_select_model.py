"""The numpy statement of through-selection (include/tdt_rt.h, "through-selection"): tdt_octree_extract_screen and
tdt_octree_edit_screen.

The world points and the projection are float32 with every operation rounded on its own, in the header's order; the rows of the view
and the three dot products are reproject_model's (view_rows, _dot), imported and not restated, so that Q exists once on this side
too.  The polygon rule runs in Python ints.  Only comparisons consume fx and fy: a NaN fails them, and np.where keeps it from the
integer cast."""
import functools

import numpy as np

from reproject_model import _dot, view_rows
from test_gpu_region_edit import apply_op

F = np.float32
RECT, POLYGON, MASK = 0, 1, 2
WINDOW = 1
MAX_VERTICES = 256
MAX_COORD = 1 << 20
REGION_PAINT, REGION_CLEAR = 2, 3


def sel_of(shape, rect=(0, 0, 0, 0), window=False, material=-1, min_distance=0.0, max_distance=np.inf):
    """struct tdt_screen_select as the dict this model reads."""
    return {"shape": int(shape), "rect": tuple(int(v) for v in rect), "flags": WINDOW if window else 0, "material": int(material),
            "min_distance": F(min_distance), "max_distance": F(max_distance)}


def world_points(k2, depth, floats):
    """k2: (..., 3) integer coordinates on the DOUBLED grid (a centre is 2k + 1, a corner 2(k + c)).  u = k2 * 2^-(depth+1) is exact;
    w = (u * scale) + min: two rounded operations.  min = floats[0:3], scale = floats[4], as tdt_pick_grid_voxel reads them."""
    floats = np.asarray(floats, F)
    u = np.asarray(k2, np.int64).astype(F) * F(2.0 ** -(depth + 1))
    assert np.array_equal(u.astype(np.float64) * 2.0 ** (depth + 1), np.asarray(k2, np.float64))          # exact
    with np.errstate(all="ignore"):
        return ((u * floats[4]).astype(F) + floats[0:3]).astype(F)


def project(w, view):
    """Q of (..., 3) float32 world points: (on, px, py, d) with on = in front and on screen, (px, py) int64 pixels (0 where not
    on) and d = w - origin."""
    ru, rv, rw, _ = view_rows(view)
    W, H = view["image_width"], view["image_height"]
    with np.errstate(all="ignore"):
        d = (np.asarray(w, F) - view["origin"]).astype(F)
        nu, nv, nw = _dot(ru, d).astype(F), _dot(rv, d).astype(F), _dot(rw, d).astype(F)
        fx = ((nu / nw).astype(F) * F(W - 1)).astype(F)
        fy = ((nv / nw).astype(F) * F(H - 1)).astype(F)
        on = (nw > 0) & (fx >= 0) & (fx < F(W)) & (fy >= 0) & (fy < F(H))
    px = np.where(on, fx, 0).astype(np.int64)
    py = np.where(on, fy, 0).astype(np.int64)
    return on, px, py, d


def pixel_in_polygon(px, py, polygon):
    """The even-odd rule at the pixel centre, in Python ints on doubled coordinates."""
    Px, Py = 2 * int(px) + 1, 2 * int(py) + 1
    n, count = len(polygon), 0
    for j in range(n):
        ax, ay = polygon[j]
        bx, by = polygon[(j + 1) % n]
        Ax, Ay, Bx, By = 2 * int(ax), 2 * int(ay), 2 * int(bx), 2 * int(by)
        if (Ay > Py) != (By > Py):
            s = (Px - Ax) * (By - Ay) - (Bx - Ax) * (Py - Ay)
            if (s < 0) if By > Ay else (s > 0):
                count += 1
    return count % 2 == 1


@functools.lru_cache(maxsize=64)
def _polygon_table(polygon, W, H):
    """inside[py][px] over the image, row by row: only the edges that cross a row's scan line are looked at per pixel (the others
    cannot count), which is pixel_in_polygon's answer."""
    table = np.zeros((H, W), bool)
    n = len(polygon)
    for py in range(H):
        Py = 2 * py + 1
        crossing = [(polygon[j], polygon[(j + 1) % n]) for j in range(n) if (2 * polygon[j][1] > Py) != (2 * polygon[(j + 1) % n][1] > Py)]
        if not crossing:
            continue
        for px in range(W):
            table[py, px] = _odd_crossings(px, Py, crossing)
    return table


def _odd_crossings(px, Py, crossing):
    Px, count = 2 * px + 1, 0
    for (ax, ay), (bx, by) in crossing:
        Ax, Ay, Bx, By = 2 * ax, 2 * ay, 2 * bx, 2 * by
        s = (Px - Ax) * (By - Ay) - (Bx - Ax) * (Py - Ay)
        if (s < 0) if By > Ay else (s > 0):
            count += 1
    return count % 2 == 1


def check_polygon(polygon):
    polygon = tuple((int(x), int(y)) for x, y in polygon)
    assert 3 <= len(polygon) <= MAX_VERTICES and all(abs(c) <= MAX_COORD for p in polygon for c in p)
    return polygon


def shape_inside(on, px, py, view, sel, polygon=None, mask=None):
    """The shape test of the pixels (px, py), where `on`."""
    if sel["shape"] == RECT:
        x0, y0, x1, y1 = sel["rect"]
        return on & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
    if sel["shape"] == POLYGON:
        return on & _polygon_table(check_polygon(polygon), view["image_width"], view["image_height"])[py, px]
    m = np.asarray(mask, F)
    assert m.shape == (view["image_height"], view["image_width"], 4)
    with np.errstate(all="ignore"):
        return on & (m[py, px, 0] > 0)                             # (NaN and -0 are outside)


def member(vox, floats, ints, view, sel, polygon=None, mask=None):
    """(selected (n,) bool, counts) over the voxels of V."""
    V = np.asarray(vox, np.int64).reshape(-1, 4)
    depth = int(ints[0])
    assert 1 <= depth <= 10 and view["image_width"] >= 2 and view["image_height"] >= 2 and view_rows(view) is not None
    k = V[:, :3]
    _, _, _, d = project(world_points(2 * k + 1, depth, floats), view)
    if sel["flags"] & WINDOW:
        corners = np.array([[c >> 2, (c >> 1) & 1, c & 1] for c in range(8)], np.int64)
        on, px, py, _ = project(world_points(2 * (k[:, None, :] + corners[None]), depth, floats), view)      # (n, 8)
        inside = shape_inside(on, px, py, view, sel, polygon, mask)
        on, inside = on.all(1), inside.all(1)
    else:
        on, px, py, _ = project(world_points(2 * k + 1, depth, floats), view)
        inside = shape_inside(on, px, py, view, sel, polygon, mask)
    inside = on & inside
    picked = inside.copy()
    if sel["material"] >= 0:
        picked &= V[:, 3] - 1 == sel["material"]
    with np.errstate(all="ignore"):
        dd = (((d[:, 2] * d[:, 2]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 0] * d[:, 0]).astype(F)).astype(F)
        lo = (F(sel["min_distance"]) * F(sel["min_distance"])).astype(F)
        hi = (F(sel["max_distance"]) * F(sel["max_distance"])).astype(F)
        picked &= (lo <= dd) & (dd <= hi)
    return picked, (len(V), int(on.sum()), int(inside.sum()), int(picked.sum()))


def extract(vox, floats, ints, view, sel, polygon=None, mask=None):
    """What tdt_octree_extract_screen returns for the Morton-sorted list `vox` of the tree, and tdt_debug_screen_counts after it."""
    V = np.asarray(vox, np.int32).reshape(-1, 4)
    picked, counts = member(V, floats, ints, view, sel, polygon, mask)
    return np.ascontiguousarray(V[picked]), counts


def edit(vox, floats, ints, view, sel, polygon, mask, op, material=0):
    """The voxel list tdt_octree_edit_screen leaves (op REGION_PAINT with brush `material`, or REGION_CLEAR), Morton-sorted, and
    the counts: the region model's paint / clear with the selected voxels as the brush."""
    assert op in (REGION_PAINT, REGION_CLEAR) and 0 <= material <= 253
    V = np.asarray(vox, np.int32).reshape(-1, 4)
    B, counts = extract(V, floats, ints, view, sel, polygon, mask)
    B = B.copy()
    B[:, 3] = material + 1
    return apply_op(V, op, B, material + 1), counts
