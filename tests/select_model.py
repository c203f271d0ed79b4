"""The numpy statement of the three contracts of screen-space selection (include/tdt_rt.h: tdt_dispatch_voxel_ids,
tdt_image_overlay, tdt_image_extract_voxels), written from the header's lines alone.  tests/test_select_model.py pins
ids_from_hits to host.pick_grid_voxel; tests/test_gpu_select.py compares the device with all three, byte for byte."""
import numpy as np

ID_DTYPE = np.dtype([("state", "<u4"), ("key", "<u4"), ("material", "<u4"), ("t", "<u4")])
VOXEL_EDGES = 1
RAY_HIT = 1


def spread3(v):
    """10 bits -> every third bit."""
    v = np.asarray(v).astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def compact3(v):
    """every third bit -> 10 bits"""
    v = np.asarray(v).astype(np.uint32) & np.uint32(0x09249249)
    v = (v | (v >> np.uint32(2))) & np.uint32(0x030C30C3)
    v = (v | (v >> np.uint32(4))) & np.uint32(0x0300F00F)
    v = (v | (v >> np.uint32(8))) & np.uint32(0x030000FF)
    v = (v | (v >> np.uint32(16))) & np.uint32(0x000003FF)
    return v


def morton(x, y, z):
    """tdt_octree_extract's key"""
    return (spread3(x) << np.uint32(2)) | (spread3(y) << np.uint32(1)) | spread3(z)


def voxel_of(key):
    """(..., 3) int32 voxel of a key"""
    key = np.asarray(key, np.uint32)
    return np.stack([compact3(key >> np.uint32(2)), compact3(key >> np.uint32(1)), compact3(key)], -1).astype(np.int32)


def ids_from_hits(hits, floats, ints, place):
    """The id texels of an array of tdt_ray_hit records (rt.RAY_HIT_DTYPE, any shape), float64 throughout: per axis
    q = (point - min) / scale + side * normal * half, k = floor(q * 2^depth); valid when 0 <= k < 2^depth on all three."""
    f = np.asarray(floats).view(np.float32).reshape(-1)
    depth = int(np.asarray(ints).view(np.int32).reshape(-1)[0])
    assert 1 <= depth <= 10 and place in (0, 1)
    cells = np.float64(1 << depth)
    half = np.float64(0.5) / cells
    side = np.float64(1.0 if place else -1.0)
    mn, scale = f[:3].astype(np.float64), np.float64(f[4])
    p, n = hits["point"].astype(np.float64), hits["normal"].astype(np.float64)
    with np.errstate(all="ignore"):
        q = (p - mn) / scale + (side * n) * half
        k = np.floor(q * cells)
        valid = ((k >= 0) & (k < cells)).all(-1)
    state = (hits["status"] == RAY_HIT) & (hits["fresh_record"] != 0) & valid
    ki = np.where(state[..., None], k, 0).astype(np.int64)
    out = np.zeros(hits.shape, ID_DTYPE)
    out["state"] = state
    out["key"] = np.where(state, morton(ki[..., 0], ki[..., 1], ki[..., 2]), 0)
    out["material"] = hits["material"]
    out["t"] = np.ascontiguousarray(hits["t"], np.float32).view(np.uint32)
    return out


def list_keys(voxels):
    """The sorted unique keys of an (n, 4) list; voxels with a coordinate outside [0, 1024) are dropped."""
    v = np.asarray(voxels, np.int64).reshape(-1, 4)
    ok = ((v[:, :3] >= 0) & (v[:, :3] < 1024)).all(1)
    v = v[ok]
    return np.unique(morton(v[:, 0], v[:, 1], v[:, 2]))


def membership(ids, voxels):
    return (ids["state"] == 1) & np.isin(ids["key"], list_keys(voxels))


def edges(ids, member, edge_width, voxel_edges):
    """edge(P): member(P) and some Q != P inside the image within edge_width (Chebyshev) that is not a member or, voxel_edges, has
    state != 1 or another key."""
    h, w = member.shape
    edge = np.zeros((h, w), bool)
    key, state1 = ids["key"], ids["state"] == 1
    for dy in range(-edge_width, edge_width + 1):
        for dx in range(-edge_width, edge_width + 1):
            if dx == 0 and dy == 0:
                continue
            ys, xs = np.arange(h) + dy, np.arange(w) + dx
            inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            yc, xc = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
            mq, kq, sq = member[yc][:, xc], key[yc][:, xc], state1[yc][:, xc]
            cond = ~mq
            if voxel_edges:
                cond = cond | ~sq | (kq != key)
            edge |= inside & cond
    return edge & member


def overlay(img, ids, voxels, style):
    """(out, member, edge, counts), counts as tdt_debug_overlay_counts gives them: style = dict(fill=(r, g, b, a), edge=(r, g, b, a), edge_width=0..4, flags=0 | VOXEL_EDGES).  fp32, every
    operation rounded on its own: out.c = (in.c * (1 - a)) + (col.c * a); alpha and non-member pixels keep their bits."""
    img = np.ascontiguousarray(img, np.float32)
    assert img.shape == ids.shape + (4,)
    ew = int(style["edge_width"])
    assert 0 <= ew <= 4 and style["flags"] in (0, VOXEL_EDGES)
    member = membership(ids, voxels)
    edge = edges(ids, member, ew, bool(style["flags"] & VOXEL_EDGES)) if ew >= 1 else np.zeros(member.shape, bool)
    fill, edg = np.asarray(style["fill"], np.float32), np.asarray(style["edge"], np.float32)
    col = np.where(edge[..., None], edg[None, None, :], fill[None, None, :]).astype(np.float32)
    a = col[..., 3:4]
    with np.errstate(all="ignore"):
        keep = np.float32(1.0) - a
        rgb = (img[..., :3] * keep) + (col[..., :3] * a)
    out = img.copy()
    out[..., :3] = np.where(member[..., None], rgb.astype(np.float32), img[..., :3])
    # (np.where copies bits: a non-member NaN keeps its payload)
    bits = out.view(np.uint32)
    bits[~member] = img.view(np.uint32)[~member]
    counts = (member.size, int((ids["state"] == 1).sum()), int(member.sum()), int(edge.sum()))
    return out, member, edge, counts


def clip_rect(rect, w, h):
    if rect is None:
        return 0, 0, w - 1, h - 1
    x0, y0, x1, y1 = (int(v) for v in rect)
    return max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)


def extract_voxels(ids, rect=None):
    """(n, 4) int32 {x, y, z, material + 1}, Morton-sorted: the distinct voxels of the state == 1 texels inside rect (inclusive,
    clipped; None: everything); of several texels with one key the last in row-major order wins.  A selected material >= 254:
    ValueError."""
    h, w = ids.shape
    x0, y0, x1, y1 = clip_rect(rect, w, h)
    if x0 > x1 or y0 > y1:
        return np.zeros((0, 4), np.int32)
    sub = ids[y0:y1 + 1, x0:x1 + 1].reshape(-1)
    sub = sub[sub["state"] == 1]
    if (sub["material"] >= 254).any():
        raise ValueError("a selected texel carries a material >= 254")
    last = {}
    for k, m in zip(sub["key"].tolist(), sub["material"].tolist()):
        last[k] = m
    keys = np.array(sorted(last), np.uint32)
    out = np.zeros((len(keys), 4), np.int32)
    if len(keys):
        out[:, :3] = voxel_of(keys)
        out[:, 3] = [last[k] + 1 for k in keys.tolist()]
    return out
