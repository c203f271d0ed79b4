"""The numpy model of stroke brushes (include/tdt_rt.h "stroke brushes"): voxel p of the grid is covered by segment (a, b) when
some point of the closed segment is within r of p — Euclidean for the round nib, Chebyshev for the cube nib — decided in int64
by the header's integer tests, vectorised over the segment's grid-clipped bounding box; of the segments covering a voxel the
highest index gives the material; the result is Morton-sorted."""
import numpy as np

SPHERE, BOX = 1, 0                     # TDT_SHAPE_SPHERE, TDT_SHAPE_BOX
COORD_MAX, RADIUS_MAX = 8192, 2048
TILE = 8


def spread3(v):
    v = np.asarray(v, np.uint64)
    k = np.zeros_like(v)
    for b in range(10):
        k |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return k


def morton(xyz):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return (spread3(xyz[:, 0]) << np.uint64(2)) | (spread3(xyz[:, 1]) << np.uint64(1)) | spread3(xyz[:, 2])


def grid(lo, hi):
    return np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)


def capsule(a, b, r, p):
    """SPHERE: with d = b - a, w = p - a, L2 = d . d, t = w . d:  t <= 0: |w|^2 <= r^2;  t >= L2: |p - b|^2 <= r^2;  otherwise
    (|w|^2 - r^2) L2 <= t^2.  bool (n,)."""
    a, b, p = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(p, np.int64).reshape(-1, 3)
    d, w = b - a, p - a
    L2, t, w2 = int(d @ d), w @ d, (w * w).sum(1)
    u = p - b
    return np.where(t <= 0, w2 <= r * r, np.where(t >= L2, (u * u).sum(1) <= r * r, (w2 - r * r) * L2 <= t * t))


def swept_box(a, b, r, p):
    """BOX: the slab test of the segment a + s d, 0 <= s <= 1, against the cube [p - r, p + r].  An axis with d_k != 0 bounds s
    to [(w_k - r) / d_k, (w_k + r) / d_k] (ends swapped where d_k < 0); the running maximum of the lower ends and minimum of the
    upper ends, starting from 0 / 1 and 1 / 1, are kept as fractions and compared by cross-multiplication.  An axis with d_k = 0
    bounds nothing but needs |w_k| <= r."""
    a, b, p = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(p, np.int64).reshape(-1, 3)
    d, w = b - a, p - a
    ok = np.ones(len(p), bool)
    lo_n, lo_d = np.zeros(len(p), np.int64), np.ones(len(p), np.int64)         # s >= lo_n / lo_d
    hi_n, hi_d = np.ones(len(p), np.int64), np.ones(len(p), np.int64)          # s <= hi_n / hi_d
    for k in range(3):
        if d[k] == 0:
            ok &= np.abs(w[:, k]) <= r
            continue
        sgn, den = (1, int(d[k])) if d[k] > 0 else (-1, -int(d[k]))
        n0, n1 = sgn * w[:, k] - r, sgn * w[:, k] + r                          # s in [n0 / den, n1 / den], den > 0
        up = n0 * lo_d > lo_n * den
        lo_n, lo_d = np.where(up, n0, lo_n), np.where(up, den, lo_d)
        down = n1 * hi_d < hi_n * den
        hi_n, hi_d = np.where(down, n1, hi_n), np.where(down, den, hi_d)
    return ok & (lo_n * hi_d <= hi_n * lo_d)


def voxel_range(a, b, r, n):
    """Inclusive voxel range (lo (3,), hi (3,)) of the segment's bounding box grown by r, inside a grid of side n."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.maximum(np.minimum(a, b) - r, 0), np.minimum(np.maximum(a, b) + r, n - 1)


def tile_candidates(a, b, r, depth):
    lo, hi = voxel_range(a, b, r, 1 << depth)
    if (lo > hi).any():
        return 0
    return int(np.prod(hi // TILE - lo // TILE + 1))


def covered_flat(a, b, r, shape, depth):
    """The voxels (n, 3) int64 of the grid one segment covers: the integer test on every voxel of the clipped box."""
    lo, hi = voxel_range(a, b, r, 1 << depth)
    if (lo > hi).any():
        return np.zeros((0, 3), np.int64)
    p = grid(lo, hi)
    return p[(capsule if shape == SPHERE else swept_box)(a, b, r, p)]


def covered(a, b, r, shape, depth, flat_limit=4096):
    """covered_flat for boxes of any size: a box of more than flat_limit voxels is cut into slabs of TILE voxels along the
    segment's longest axis k.  A covered voxel p has a point q of the segment with |p_j - q_j| <= r on every axis (both metrics),
    so a slab k0..k1 needs only the piece of the segment with q_k in [k0 - r, k1 + r], and of the other axes only that piece's
    extent grown by r (and by one voxel more, against the rounding of the piece's ends).  The test itself stays the integer one."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    lo, hi = voxel_range(a, b, r, 1 << depth)
    if (lo > hi).any():
        return np.zeros((0, 3), np.int64)
    d = b - a
    k = int(np.argmax(np.abs(d)))
    if d[k] == 0 or int(np.prod(hi - lo + 1)) <= flat_limit:
        return covered_flat(a, b, r, shape, depth)
    test = capsule if shape == SPHERE else swept_box
    out = [np.zeros((0, 3), np.int64)]
    for k0 in range(int(lo[k]), int(hi[k]) + 1, TILE):
        k1 = min(k0 + TILE - 1, int(hi[k]))
        s0, s1 = sorted(((k0 - r - a[k]) / d[k], (k1 + r - a[k]) / d[k]))
        s0, s1 = max(s0, 0.0), min(s1, 1.0)
        if s0 > s1:
            continue
        slo, shi = lo.copy(), hi.copy()
        slo[k], shi[k] = k0, k1
        for j in range(3):
            if j != k:
                e0, e1 = sorted((a[j] + s0 * d[j], a[j] + s1 * d[j]))
                slo[j], shi[j] = max(lo[j], int(np.floor(e0)) - r - 1), min(hi[j], int(np.ceil(e1)) + r + 1)
        if (slo > shi).any():
            continue
        p = grid(slo, shi)
        out.append(p[test(a, b, r, p)])
    return np.concatenate(out)


def segments_of(n_points, segments=None):
    """The (m, 2) segment list a stroke stands for: the given one, or the polyline of the points (one point: one dab)."""
    if segments is not None:
        return np.asarray(segments, np.int64).reshape(-1, 2)
    if n_points <= 1:
        return np.zeros((n_points, 2), np.int64)
    i = np.arange(n_points - 1, dtype=np.int64)
    return np.stack([i, i + 1], 1)


def voxelize(points, radius, depth, segments=None, materials=None, material=0, shape=SPHERE):
    """(n, 4) int32 {x, y, z, material + 1}, Morton-sorted and unique: tdt_voxelize_stroke."""
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    seg = segments_of(len(pts), segments)
    mats = np.full(len(seg), material + 1, np.int64) if materials is None else np.asarray(materials, np.int64)
    vox, who = [], []
    for s, (i, j) in enumerate(seg):
        c = covered(pts[i], pts[j], radius, shape, depth)
        vox.append(c)
        who.append(np.full(len(c), s, np.int64))
    if not vox or not sum(len(c) for c in vox):
        return np.zeros((0, 4), np.int32)
    vox, who = np.concatenate(vox), np.concatenate(who)
    key = morton(vox)
    order = np.lexsort((who, key))                  # by key, then by segment: the last of a run is the highest segment
    key, vox, who = key[order], vox[order], who[order]
    last = np.append(key[1:] != key[:-1], True)
    return np.ascontiguousarray(np.concatenate([vox[last], mats[who[last]][:, None]], 1).astype(np.int32))


def intersect(V, B):
    """V's voxels (with V's materials) that B holds: tdt_octree_extract_stroke."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    return np.ascontiguousarray(V[np.isin(morton(V[:, :3]), morton(np.asarray(B).reshape(-1, 4)[:, :3]))])


def random_stroke(rng, count, n, reach=None):
    """A polyline of count segments whose points lie between -reach and n - 1 + reach (default n // 2): steps of mixed lengths, from
    a voxel to a jump anywhere in that range (a step that would leave it is a jump too); (points (count + 1, 3) int32, materials
    (count,) int32)."""
    reach = n // 2 if reach is None else reach
    lo, hi = -reach, n - 1 + reach
    pts = [rng.integers(lo, hi + 1, 3)]
    for i in range(count):
        span = int(rng.choice([1, 3, max(n // 4, 1), 0]))
        q = pts[-1] + rng.integers(-span, span + 1, 3)
        if span == 0 or (q < lo).any() or (q > hi).any():
            q = rng.integers(lo, hi + 1, 3)
        pts.append(q)
    return np.stack(pts).astype(np.int32), rng.integers(1, 255, count).astype(np.int32)


def stroke_from_picks(voxels):
    """Renderer.stroke's points and segments from one entry per pixel: a (3,) voxel for a hit, None for a miss.  Consecutive hits
    are joined, a miss breaks the stroke, a hit between misses is a dab (i, i), listed after the joins."""
    points, segments, prev = [], [], None
    for v in voxels:
        if v is None:
            prev = None
            continue
        points.append(np.asarray(v, np.int32))
        if prev is not None:
            segments.append((prev, len(points) - 1))
        prev = len(points) - 1
    joined = {i for g in segments for i in g}
    segments += [(i, i) for i in range(len(points)) if i not in joined]
    return np.asarray(points, np.int32).reshape(-1, 3), np.asarray(segments, np.uint32).reshape(-1, 2)
