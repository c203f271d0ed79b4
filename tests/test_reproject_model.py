"""The reprojection model (tests/reproject_model.py) on a hand-made scene: a fronto-parallel wall z = -4 and a floor y = -1, seen
by pinhole views whose rays go through pixel centres (built in float64, rounded once).  With the numbers below — a 17x13 image, a
viewport of 2 x 1.5 at focal length 1 — a pixel is 0.5 wide on the wall, rows 0..3 see the floor and rows 4..12 the wall."""
import numpy as np

import reproject_model as model
from denoise_model import GUIDE_DTYPE

F = np.float32
W, H = 17, 13
WALL_Z, FLOOR_Y = -4.0, -1.0
WALL = (15, 2, F(WALL_Z))             # kind = 1 + face code of normal (0, 0, +1); material; plane
FLOOR = (17, 3, F(FLOOR_Y))           # normal (0, +1, 0)
SPP = 4


def view(origin=(0.0, 0.0, 0.0), mirrored=False):
    o = np.array(origin, np.float64)
    hor, ver = np.array([2.0, 0, 0]), np.array([0, 1.5, 0])
    llc = o - hor / 2 - ver / 2 + np.array([0, 0, -1.0])
    if mirrored:                      # the same picture with x running the other way: a negative determinant
        llc, hor = llc + hor, -hor
    return model.view_of(o, llc, hor, ver, W, H)


def frame(v):
    """(rays (H, W, 6) float32, guide (H, W)) of what view v sees, the rays through pixel centres."""
    o = v["origin"].astype(np.float64)
    rays = np.zeros((H, W, 6), np.float64)
    guide = np.zeros((H, W), GUIDE_DTYPE)
    for y in range(H):
        for x in range(W):
            d = (v["lower_left_corner"] + (x + 0.5) / (W - 1) * v["horizontal"].astype(np.float64)
                 + (y + 0.5) / (H - 1) * v["vertical"].astype(np.float64) - o)
            d /= np.sqrt((d * d).sum())
            hits = []
            if d[2] < 0 and o[2] > WALL_Z:
                hits.append(((WALL_Z - o[2]) / d[2], WALL))
            if d[1] < 0:
                hits.append(((FLOOR_Y - o[1]) / d[1], FLOOR))
            rays[y, x] = (*o, *d)
            if hits:
                t, key = min(hits, key=lambda h: h[0])
                guide[y, x] = (*key, t)
    return rays.astype(F), guide


def history(seed, n=8.0):
    rng = np.random.default_rng(seed)
    h = rng.random((H, W, 4)).astype(F)
    h[..., 3] = F(n)
    return h


def sums_of(seed):
    return np.random.default_rng(seed).random((H, W, 4)).astype(F)


def only(guide, key):
    g = guide.copy()
    g[g["kind"] != key[0]] = (0, 0, 0, 0)
    return g


def test_the_scene_is_what_the_docstring_says():
    _, g = frame(view())
    assert (g["kind"][:4] == FLOOR[0]).all() and (g["kind"][4:] == WALL[0]).all()


def test_identical_views_map_every_keyed_pixel_to_itself():
    v = view()
    rays, g = frame(v)
    g[6, 5] = (0, 0, 0, 0)                                            # a hole: passes through
    ph, s = history(1), sums_of(2)
    hist, mean, Q, found, counts = model.reproject(rays, g, s, SPP, v, g, ph, 64.0)
    keyed = g["kind"] != 0
    ys, xs = np.mgrid[:H, :W]
    assert found[keyed].all() and not found[~keyed].any()
    assert (Q[..., 0][keyed] == xs[keyed]).all() and (Q[..., 1][keyed] == ys[keyed]).all()
    assert counts == (int(keyed.sum()), int(keyed.sum()), 0, 0)
    want = (s[..., :3] + ph[..., :3]).astype(F)
    assert (hist[..., :3][keyed] == want[keyed]).all() and (hist[..., 3][keyed] == F(12)).all()
    assert hist[6, 5].tolist() == [*s[6, 5, :3].tolist(), 4.0]
    assert (mean[..., :3] == (hist[..., :3] / hist[..., 3:]).astype(F)).all() and (mean[..., 3] == 1).all()
    # no history at all: the sums and spp
    hist0, _, _, found0, counts0 = model.reproject(rays, g, s, SPP, None, None, None, 64.0)
    assert not found0.any() and counts0 == (int(keyed.sum()), 0, 0, 0)
    assert (hist0[..., :3] == s[..., :3]).all() and (hist0[..., 3] == 4).all()


def test_a_sideways_shift_by_whole_pixels_of_the_wall():
    k = 3
    cur, old = view(), view(origin=(-k * 0.5, 0.0, 0.0))              # a pixel is 0.5 wide at the wall's depth
    rays, g = frame(cur)
    g = only(g, WALL)
    _, pg = frame(old)
    hist, _, Q, found, counts = model.reproject(rays, g, sums_of(3), SPP, old, pg, history(4), 64.0)
    ys, xs = np.mgrid[:H, :W]
    wall = g["kind"] != 0
    inside = wall & (xs + k < W)
    assert found[inside].all() and not found[wall & ~inside].any()
    assert (Q[..., 0][inside] == xs[inside] + k).all() and (Q[..., 1][inside] == ys[inside]).all()
    n_wall_rows = H - 4
    assert counts == (n_wall_rows * W, n_wall_rows * (W - k), 0, n_wall_rows * k)


def test_a_point_behind_the_old_camera_is_rejected_by_nw():
    cur, old = view(), view(origin=(0.0, 0.0, -8.0))                  # the old eye stood behind the wall, looking away from it
    rays, g = frame(cur)
    g = only(g, WALL)
    pg = np.zeros((H, W), GUIDE_DTYPE)
    pg[:] = (*WALL, 1.0)                                              # the key would match wherever the mirror image landed
    _, _, _, found, counts = model.reproject(rays, g, sums_of(5), SPP, old, pg, history(6), 64.0)
    n = int((g["kind"] != 0).sum())
    assert n and not found.any() and counts == (n, 0, 0, n)


def test_keys_differing_by_an_ulp_or_in_material_are_rejected():
    v = view()
    rays, g = frame(v)
    keyed = int((g["kind"] != 0).sum())
    for change in ("plane", "material"):
        pg = g.copy()
        if change == "plane":
            pg["plane"] = np.nextafter(pg["plane"], F(np.inf))
        else:
            pg["material"] += 1
        hist, _, _, found, counts = model.reproject(rays, g, sums_of(7), SPP, v, pg, history(8), 64.0)
        assert not found.any() and counts == (keyed, 0, keyed, 0), change
        assert (hist[..., 3] == 4).all()
    pg = g.copy()                                                     # one texel only
    pg["plane"][7, 7] = np.nextafter(pg["plane"][7, 7], F(-np.inf))
    _, _, _, found, counts = model.reproject(rays, g, sums_of(7), SPP, v, pg, history(8), 64.0)
    assert not found[7, 7] and counts == (keyed, keyed - 1, 1, 0)


def test_sample_counts_that_are_not_positive_are_rejected():
    v = view()
    rays, g = frame(v)
    ph, s = history(9), sums_of(10)
    ph[5, 5, 3], ph[5, 6, 3], ph[5, 7, 3] = 0.0, -1.0, np.nan
    ph[5, 7, :3] = np.nan                                             # must not reach the sums
    hist, mean, _, found, counts = model.reproject(rays, g, s, SPP, v, g, ph, 64.0)
    n = W * H
    assert not found[5, 5:8].any() and counts == (n, n - 3, 3, 0)
    assert (hist[5, 5:8, :3] == s[5, 5:8, :3]).all() and (hist[5, 5:8, 3] == 4).all()
    assert np.isfinite(mean).all()


def test_the_cap():
    v = view()
    rays, g = frame(v)
    ph, s = history(11), sums_of(12)
    cap = F(6.5)
    under, over = np.nextafter(cap, F(0)), np.nextafter(cap, F(np.inf))
    ph[8, 2, 3], ph[8, 3, 3], ph[8, 4, 3], ph[8, 5, 3] = under, cap, over, 100.0
    hist, _, _, found, _ = model.reproject(rays, g, s, SPP, v, g, ph, cap)
    assert found.all()
    for x, hn in ((2, under), (3, cap)):                              # not over the cap: the history as it is
        assert (hist[8, x, :3] == (s[8, x, :3] + ph[8, x, :3]).astype(F)).all() and hist[8, x, 3] == F(F(4) + hn)
    for x, hn in ((4, over), (5, F(100.0))):
        scale = F(cap / hn)
        assert (hist[8, x, :3] == (s[8, x, :3] + (ph[8, x, :3] * scale).astype(F)).astype(F)).all() and hist[8, x, 3] == F(10.5)
    assert (hist[..., 3][ph[..., 3] == 8] == F(10.5)).all()          # 8 samples of history against a cap of 6.5


def test_a_mirrored_view_has_its_rows_negated():
    plain, mirrored = view(), view(mirrored=True)
    ru, rv, rw, sign = model.view_rows(plain)
    mu, mv, mw, msign = model.view_rows(mirrored)
    # a camera looking down -z with x to the right has (a, b, c) left-handed: its determinant is the negative one
    assert sign == -1 and msign == 1
    for v, (qu, qv, qw), sg in ((plain, (ru, rv, rw), -1.0), (mirrored, (mu, mv, mw), 1.0)):
        c = (v["lower_left_corner"] - v["origin"]).astype(np.float64)
        a, b = v["horizontal"].astype(np.float64), v["vertical"].astype(np.float64)
        assert (qw == (sg * np.cross(a, b)).astype(F)).all() and (qu == (sg * np.cross(b, c)).astype(F)).all()
        assert (qv == (sg * np.cross(c, a)).astype(F)).all()
        assert float(c @ qw) > 0                                     # the determinant after the fix: nw > 0 in front of the eye
    # the current frame (plain view) into the mirrored old view: column x lands in column W - 2 - x (fx = W - 1 - (x + 0.5))
    rays, g = frame(plain)
    g = only(g, WALL)
    pg = np.zeros((H, W), GUIDE_DTYPE)
    pg[:] = (*WALL, 1.0)
    _, _, Q, found, counts = model.reproject(rays, g, sums_of(13), SPP, mirrored, pg, history(14), 64.0)
    ys, xs = np.mgrid[:H, :W]
    wall = g["kind"] != 0
    inside = wall & (xs <= W - 2)
    assert found[inside].all() and (Q[..., 0][inside] == W - 2 - xs[inside]).all() and (Q[..., 1][inside] == ys[inside]).all()
    assert counts == ((H - 4) * W, (H - 4) * (W - 1), 0, H - 4)
    assert model.view_rows(model.view_of((0, 0, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0), W, H)) is None     # c = 0: no determinant
