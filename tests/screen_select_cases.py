"""Inputs of the through-selection suites (tests/test_screen_select_model.py on the CPU, tests/test_gpu_screen_select.py on the GPU):
trees whose voxel counts sit on the wave and block edges of the kernel's ballots and counts, the three image sizes, three cameras per
tree (outside the grid, inside it, and with its origin exactly on a voxel's centre) and the screen shapes.  Plain numpy."""
import functools

import numpy as np

import screen_select_model as model
import tree_cases
from reproject_model import view_of

F = np.float32
IMAGES = ((2, 2), (33, 17), (64, 48))
# OctreeFloats of two grids: the unit cube at the origin, and one whose min and scale round in every operation
FLOATS = {"unit": np.array([0, 0, 0, 0, 1, 1, 1 / 64], F), "odd": np.array([-1.3, 0.7, -0.45, 0, 2.7, 1 / 2.7, 1 / 64], F)}


@functools.lru_cache(maxsize=None)
def trees():
    """name -> (depth, V): V Morton-sorted {x, y, z, material + 1}.  |V| = 1, 63, 64, 65, 255, 256, 257 (one voxel either side of a
    wave and of a block), 2048 and sparse_d10's 16 393; n256 is of one material."""
    out = {"n1": (3, tree_cases.random_voxels(np.random.default_rng(31), 3, 1))}
    for n in (63, 64, 65):
        _, depth, v = tree_cases.family(f"capacity-{n}")
        out[f"n{n}"] = (depth, v)
    for n in (255, 256, 257):
        v = tree_cases.random_voxels(np.random.default_rng(3000 + n), 5, n).copy()
        if n == 256:
            v[:, 3] = 10
        out[f"n{n}"] = (5, v)
    _, depth, v = tree_cases.family("level-count-edge-2048")
    out["n2048"] = (depth, v)
    out["d10"] = (10, tree_cases.sparse_d10())
    return {k: (d, tree_cases.sort_vox(v)) for k, (d, v) in out.items()}


def ints_of(depth):
    return np.array([depth, 64, 64], np.int32)


def look(origin, yaw, pitch, half_w, half_h, W, H):
    """A pinhole view at `origin` looking along (sin yaw cos pitch, sin pitch, cos yaw cos pitch), the image plane at distance 1."""
    f = np.array([np.sin(yaw) * np.cos(pitch), np.sin(pitch), np.cos(yaw) * np.cos(pitch)])
    r = np.cross([0.0, 1.0, 0.0], f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    o = np.asarray(origin, np.float64)
    return view_of(o.astype(F), o + f - half_w * r - half_h * u, 2 * half_w * r, 2 * half_h * u, W, H)


def cameras(V, depth, floats, W, H):
    """name -> view.  outside: in front of the grid, a field of view that cuts some of it off; inside: near the grid's middle, so
    that part of the tree is behind it; centre: the origin is bit for bit the world point of the centre of V's middle voxel, looking
    along +z, so that voxel has nw = 0 and 0 / 0 in Q."""
    floats = np.asarray(floats, F)
    mn, s = floats[:3].astype(np.float64), float(floats[4])
    mid = model.world_points(2 * V[len(V) // 2, :3].astype(np.int64) + 1, depth, floats)
    return {"outside": look(mn + s * np.array([0.45, 0.6, -0.9]), 0.1, -0.05, 0.4, 0.3, W, H),
            "inside": look(mn + s * np.array([0.52, 0.47, 0.41]), -0.4, 0.2, 1.0, 0.9, W, H),
            "centre": view_of(mid, mid.astype(np.float64) + [-0.9, -0.7, 1.0], [1.8, 0, 0], [0, 1.4, 0], W, H)}


def rect_polygon(x0, y0, x1, y1):
    """The polygon that is the RECT x0..x1, y0..y1."""
    return [(x0, y0), (x1 + 1, y0), (x1 + 1, y1 + 1), (x0, y1 + 1)]


def rect_mask(x0, y0, x1, y1, W, H):
    m = np.zeros((H, W, 4), F)
    m[max(y0, 0): max(y1 + 1, 0), max(x0, 0): max(x1 + 1, 0), 0] = 1.0
    return m


def circle(cx, cy, r, n=256):
    """n integer vertices on a circle (neighbours may coincide: an edge of no length counts nothing)."""
    t = 2 * np.pi * np.arange(n) / n
    return [(int(round(cx + r * np.cos(a))), int(round(cy + r * np.sin(a)))) for a in t]


def random_mask(W, H, seed):
    """About half the texels inside; NaN, -0.0, a denormal, a negative value and +inf among the red channels, and junk in the other
    channels, which are not read."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((H, W, 4)).astype(F)
    red = m[..., 0].reshape(-1)
    special = np.array([np.nan, -0.0, 1e-42, -1e-42, -3.0, np.inf, 0.0, -np.nan], F)
    red[rng.permutation(red.size)[: len(special)]] = special[: red.size]
    m[..., 0] = red.reshape(H, W)
    return m


def shapes(W, H, seed=0):
    """name -> (sel keywords, polygon, mask): every shape of the contract for a W x H image."""
    x0, y0, x1, y1 = W // 4, H // 5, W - 1 - W // 3, H - 1 - H // 4
    out = {
        "rect-all": (dict(shape=model.RECT, rect=(0, 0, W - 1, H - 1)), None, None),
        "rect-pixel": (dict(shape=model.RECT, rect=(W // 2, H // 2, W // 2, H // 2)), None, None),
        "rect-clipped": (dict(shape=model.RECT, rect=(-5, H // 2, W + 7, 2 * H)), None, None),
        "rect-empty": (dict(shape=model.RECT, rect=(W // 2, 0, W // 2 - 1, H - 1)), None, None),
        "rect-part": (dict(shape=model.RECT, rect=(x0, y0, x1, y1)), None, None),
        "poly-rect": (dict(shape=model.POLYGON), rect_polygon(x0, y0, x1, y1), None),
        "poly-triangle": (dict(shape=model.POLYGON), [(0, 0), (W, H // 3), (W // 3, H)], None),
        "poly-outside": (dict(shape=model.POLYGON), [(-40, -30), (2 * W, H // 4), (W // 2, H // 2), (W // 3, 3 * H), (-W, H // 2)], None),
        "poly-bowtie": (dict(shape=model.POLYGON), [(0, 0), (W, H), (W, 0), (0, H)], None),
        "poly-circle": (dict(shape=model.POLYGON), circle(W / 2, H / 2, min(W, H) * 0.45), None),
        "mask-rect": (dict(shape=model.MASK), None, rect_mask(x0, y0, x1, y1, W, H)),
        "mask-random": (dict(shape=model.MASK), None, random_mask(W, H, 77 + seed)),
    }
    return out
