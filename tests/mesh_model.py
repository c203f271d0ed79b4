"""The numpy model of triangle-mesh voxelisation (include/tdt_rt.h "triangle meshes"): a closed triangle covers a closed voxel
cube iff no axis among the 13 (3 box axes, the normal, 9 edge x box-axis products) separates them, in int64; of the triangles
covering a voxel the highest index gives the material; the result is Morton-sorted.  Hierarchical like the kernels (8^3-voxel
tiles first, then the voxels of the surviving tiles) so a grid-spanning triangle takes seconds, but every axis is evaluated
the plain way: all three vertices and the box's extreme corners projected on it."""
import numpy as np

FRAC = 6
UNIT = 1 << FRAC
COORD_MAX = 1 << 18
TILE = 8
KINDS = ("general", "lattice", "segment", "point", "plane", "collinear")


def spread3(v):
    v = np.asarray(v, np.uint64)
    k = np.zeros_like(v)
    for b in range(10):
        k |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return k


def morton(xyz):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return (spread3(xyz[:, 0]) << np.uint64(2)) | (spread3(xyz[:, 1]) << np.uint64(1)) | spread3(xyz[:, 2])


def axes_of(tri):
    """The 13 candidate separating axes of one triangle (3, 3) int64, as a (13, 3) int64 array."""
    tri = np.asarray(tri, np.int64)
    e = np.stack([tri[1] - tri[0], tri[2] - tri[1], tri[0] - tri[2]])
    unit = np.eye(3, dtype=np.int64)
    out = [unit[0], unit[1], unit[2], np.cross(e[0], e[1])]
    for i in range(3):
        for k in range(3):
            out.append(np.cross(e[i], unit[k]))
    return np.stack(out).astype(np.int64)


def overlap(tri, corners, side):
    """Closed triangle against the closed boxes [c, c + side]^3 (units), c = corners (n, 3): bool (n,)."""
    tri = np.asarray(tri, np.int64)
    c = np.asarray(corners, np.int64).reshape(-1, 3)
    hit = np.ones(len(c), bool)
    for a in axes_of(tri):
        t = tri @ a
        base = c @ a
        lo = base + side * int(np.minimum(a, 0).sum())
        hi = base + side * int(np.maximum(a, 0).sum())
        hit &= ~((t.max() < lo) | (t.min() > hi))
    return hit


def voxel_range(tri, n):
    """Inclusive voxel range (lo (3,), hi (3,)) the triangle's bounding box touches inside a grid of side n; a coordinate on a
    voxel boundary touches both neighbours."""
    tri = np.asarray(tri, np.int64)
    lo = np.floor_divide(tri.min(0) - 1, UNIT)
    hi = np.floor_divide(tri.max(0), UNIT)
    return np.maximum(lo, 0), np.minimum(hi, n - 1)


def grid(lo, hi):
    return np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)


def tile_candidates(tri, depth):
    lo, hi = voxel_range(tri, 1 << depth)
    if (lo > hi).any():
        return 0
    return int(np.prod(hi // TILE - lo // TILE + 1))


def covered(tri, depth, stats=None):
    """The voxels (n, 3) int64 of the grid one triangle covers."""
    lo, hi = voxel_range(tri, 1 << depth)
    if (lo > hi).any():
        return np.zeros((0, 3), np.int64)
    tiles = grid(lo // TILE, hi // TILE)
    keep = tiles[overlap(tri, tiles * (TILE * UNIT), TILE * UNIT)]
    if stats is not None:
        stats["tiles"] = stats.get("tiles", 0) + len(tiles)
        stats["kept"] = stats.get("kept", 0) + len(keep)
    if not len(keep):
        return np.zeros((0, 3), np.int64)
    cell = grid(np.zeros(3, np.int64), np.full(3, TILE - 1, np.int64))
    vox = (keep[:, None, :] * TILE + cell[None]).reshape(-1, 3)
    vox = vox[((vox >= lo) & (vox <= hi)).all(1)]
    if stats is not None:
        stats["tests"] = stats.get("tests", 0) + len(vox)
    return vox[overlap(tri, vox * UNIT, UNIT)]


def voxelize(vertices, triangles, depth, materials=None, material=0, stats=None):
    """(n, 4) int32 {x, y, z, material + 1}, Morton-sorted and unique: tdt_voxelize_triangles."""
    v = np.asarray(vertices, np.int64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    mats = np.full(len(t), material + 1, np.int64) if materials is None else np.asarray(materials, np.int64)
    vox, who = [], []
    for i, idx in enumerate(t):
        c = covered(v[idx], depth, stats)
        vox.append(c)
        who.append(np.full(len(c), i, np.int64))
    if not vox or not sum(len(c) for c in vox):
        return np.zeros((0, 4), np.int32)
    vox, who = np.concatenate(vox), np.concatenate(who)
    if stats is not None:
        stats["pairs"] = len(vox)
    key = morton(vox)
    order = np.lexsort((who, key))                  # by key, then by triangle: the last of a run is the highest triangle
    key, vox, who = key[order], vox[order], who[order]
    last = np.append(key[1:] != key[:-1], True)
    return np.ascontiguousarray(np.concatenate([vox[last], mats[who[last]][:, None]], 1).astype(np.int32))


def voxelize_many(vertices, triangles, depth, materials=None, material=0, flat_limit=4096, chunk=1 << 22):
    """voxelize() for meshes of very many triangles: the same 13 axes, evaluated for whole batches of (triangle, voxel of its
    grid-clipped bounding box) pairs at once; a triangle whose box holds more than flat_limit voxels takes covered()."""
    v = np.asarray(vertices, np.int64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if not len(t):
        return np.zeros((0, 4), np.int32)
    mats = np.full(len(t), material + 1, np.int64) if materials is None else np.asarray(materials, np.int64)
    n = 1 << depth
    tri = v[t]                                                  # (m, 3, 3)
    lo = np.maximum(np.floor_divide(tri.min(1) - 1, UNIT), 0)
    hi = np.minimum(np.floor_divide(tri.max(1), UNIT), n - 1)
    ext = np.maximum(hi - lo + 1, 0)
    cnt = ext.prod(1)
    e = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2]], 1)
    unit = np.eye(3, dtype=np.int64)
    axes = [np.broadcast_to(unit[k], (len(t), 3)) for k in range(3)] + [np.cross(e[:, 0], e[:, 1])]
    axes += [np.cross(e[:, i], unit[k]) for i in range(3) for k in range(3)]
    axes = np.stack(axes, 1).astype(np.int64)                   # (m, 13, 3)
    proj = np.einsum("mvk,mak->mav", tri, axes)                 # (m, 13, 3 vertices)
    tmin, tmax = proj.min(2), proj.max(2)
    neg, pos = np.minimum(axes, 0).sum(2) * UNIT, np.maximum(axes, 0).sum(2) * UNIT
    vox, who = [], []
    for i in np.flatnonzero(cnt > flat_limit):
        c = covered(tri[i], depth)
        vox.append(c)
        who.append(np.full(len(c), i, np.int64))
    small = np.flatnonzero((cnt > 0) & (cnt <= flat_limit))
    ends = np.cumsum(cnt[small])
    start = 0
    while start < len(small):
        stop = max(int(np.searchsorted(ends, (ends[start - 1] if start else 0) + chunk, side="right")), start + 1)
        ids = small[start:stop]
        c = cnt[ids]
        owner = np.repeat(ids, c)
        local = np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c)
        ex = ext[owner]
        p = np.stack([local // (ex[:, 1] * ex[:, 2]), (local // ex[:, 2]) % ex[:, 1], local % ex[:, 2]], 1) + lo[owner]
        hit = np.ones(len(p), bool)
        for a in range(13):
            base = (p * UNIT * axes[owner, a]).sum(1)
            hit &= ~((tmax[owner, a] < base + neg[owner, a]) | (tmin[owner, a] > base + pos[owner, a]))
        vox.append(p[hit])
        who.append(owner[hit])
        start = stop
    vox, who = np.concatenate(vox), np.concatenate(who)
    if not len(vox):
        return np.zeros((0, 4), np.int32)
    key = morton(vox)
    order = np.lexsort((who, key))
    key, vox, who = key[order], vox[order], who[order]
    last = np.append(key[1:] != key[:-1], True)
    return np.ascontiguousarray(np.concatenate([vox[last], mats[who[last]][:, None]], 1).astype(np.int32))


def random_triangles(rng, count, n, kinds=KINDS):
    """count triangles, their kinds cycling through `kinds`, with vertices from -1 to n + 1 voxels: (vertices (3 count, 3) int32 in
    units, triangles (count, 3) uint32, kind names).  Sizes vary from below a voxel to the whole grid."""
    lo, hi = -UNIT, (n + 1) * UNIT
    verts, names = [], []
    for i in range(count):
        kind = kinds[i % len(kinds)]
        a = rng.integers(lo, hi + 1, 3)
        span = int(rng.choice([UNIT // 2, 2 * UNIT, 6 * UNIT, max(n * UNIT // 2, UNIT), n * UNIT + 2 * UNIT]))

        def near(p):
            return np.clip(p + rng.integers(-span, span + 1, 3), lo, hi)

        if kind == "general":
            tri = [a, near(a), near(a)]
        elif kind == "lattice":
            a = (a // UNIT) * UNIT
            tri = [a, (near(a) // UNIT) * UNIT, (near(a) // UNIT) * UNIT]
        elif kind == "segment":
            b = near(a)
            tri = [a, b, b if i & 1 else a]
        elif kind == "point":
            if i & 1:
                a = (a // UNIT) * UNIT
            tri = [a, a, a]
        elif kind == "plane":
            axis = int(rng.integers(0, 3))
            a[axis] = int(rng.integers(0, n + 1)) * UNIT
            b, c = near(a), near(a)
            b[axis] = c[axis] = a[axis]
            tri = [a, b, c]
        else:                                          # collinear, three distinct points on one line where the range allows
            d = rng.integers(-span // 4 - 1, span // 4 + 2, 3)
            if i & 1:
                d = (d // UNIT) * UNIT + np.array([UNIT, 0, 0]) * (1 if not d.any() else 0)
            tri = [a, np.clip(a + d, lo - span, hi + span), np.clip(a + 3 * d, lo - 3 * span, hi + 3 * span)]
            if not (np.cross(tri[1] - tri[0], tri[2] - tri[0]) == 0).all():       # a clip bent it: fall back to a plain segment
                tri = [a, a + d, a]
        verts += [np.asarray(p, np.int64) for p in tri]
        names.append(kind)
    v = np.stack(verts).astype(np.int32)
    assert np.abs(v).max() <= COORD_MAX
    return v, np.arange(3 * count, dtype=np.uint32).reshape(-1, 3), names


def oblique_triangle():
    """The depth-9 triangle of the contract: 2^27 voxels in its bounding box, 264,697 covered."""
    v = np.array([[0, 0, 0], [512, 256, 512], [256, 512, 512]], np.int32) * UNIT
    return v, np.array([[0, 1, 2]], np.uint32)


def uv_sphere(centre, radius, stacks, slices):
    """A UV sphere in float voxel coordinates: (vertices (n, 3) float32, triangles (m, 3) uint32), 2 slices (stacks - 1) triangles."""
    th = np.linspace(0.0, np.pi, stacks + 1)[1:-1]
    ph = np.linspace(0.0, 2 * np.pi, slices, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], -1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radius + np.asarray(centre, np.float64)
    tris = []
    south = 1 + (stacks - 1) * slices
    for j in range(slices):
        k = (j + 1) % slices
        tris.append((0, 1 + j, 1 + k))
        tris.append((south, 1 + (stacks - 2) * slices + k, 1 + (stacks - 2) * slices + j))
    for i in range(stacks - 2):
        a, b = 1 + i * slices, 1 + (i + 1) * slices
        for j in range(slices):
            k = (j + 1) % slices
            tris += [(a + j, b + j, b + k), (a + j, b + k, a + k)]
    return v.astype(np.float32), np.array(tris, np.uint32)


def torus(centre, major, minor, rings, sides):
    """A torus around the z axis in float voxel coordinates: 2 rings sides triangles."""
    u = np.linspace(0.0, 2 * np.pi, rings, endpoint=False)[:, None]
    w = np.linspace(0.0, 2 * np.pi, sides, endpoint=False)[None, :]
    r = major + minor * np.cos(w)
    v = np.stack([r * np.cos(u), r * np.sin(u), minor * np.sin(w) * np.ones_like(u)], -1).reshape(-1, 3) + np.asarray(centre, np.float64)
    tris = []
    for i in range(rings):
        for j in range(sides):
            a, b = i * sides + j, i * sides + (j + 1) % sides
            c, d = ((i + 1) % rings) * sides + j, ((i + 1) % rings) * sides + (j + 1) % sides
            tris += [(a, c, d), (a, d, b)]
    return v.astype(np.float32), np.array(tris, np.uint32)


def quantize(xyz, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """tdt_mesh_quantize in numpy: float32 -> float64, * scale + offset, * 64, round half to even."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    return np.rint((p * np.float64(scale) + np.asarray(offset, np.float64)) * 64.0).astype(np.int64)


def fit(xyz, lo, hi):
    """tdt_mesh_fit in numpy: the uniform scale and the offset that centre the bounding box of xyz in the voxel box lo..hi
    inclusive (the continuous box [lo, hi + 1]) with the longest edge spanning it; a zero-extent mesh: scale 1."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64) + 1.0
    mn, mx = p.min(0), p.max(0)
    ext = mx - mn
    room = hi - lo
    scale = 1.0
    if ext.max() > 0:
        scale = min(room[a] / ext[a] for a in range(3) if ext[a] > 0)
    offset = (lo + hi) * 0.5 - (mn + mx) * 0.5 * scale
    return float(scale), offset
