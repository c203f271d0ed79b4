"""The numpy statement of temporal reprojection (include/tdt_rt.h, "temporal reprojection").

view_rows: the per-call part, in float64 with one rounding per operation, then rounded to float32.  reproject: the per-pixel part
in float32 with the operation order the header fixes, so that the GPU's bytes can be compared with it bit for bit.  The primary
rays are an INPUT (on the GPU tests they are what pick returns; on the CPU they are made by hand): nothing here restates the
sampler's hash.  Skipped branches go through np.where, as in denoise_model.py: a NaN behind a rejected history texel must not
reach the sums."""
import numpy as np

F = np.float32


def view_of(origin, lower_left_corner, horizontal, vertical, image_width, image_height):
    """A view as the dict this model reads (rt.VIEW's fields)."""
    return {"origin": np.asarray(origin, F), "lower_left_corner": np.asarray(lower_left_corner, F), "horizontal": np.asarray(horizontal, F),
            "vertical": np.asarray(vertical, F), "image_width": int(image_width), "image_height": int(image_height)}


def view_from_ctypes(v):
    return view_of(list(v.origin), list(v.lower_left_corner), list(v.horizontal), list(v.vertical), v.image_width, v.image_height)


def _cross(u, w):
    out = np.zeros(3, np.float64)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        p = u[j] * w[k]
        q = u[k] * w[j]
        out[i] = p - q
    return out


def view_rows(view):
    """(Ru, Rv, Rw) as float32 vectors and the determinant's sign before the fix (+1 / -1); None when the view is degenerate."""
    a = view["horizontal"].astype(np.float64)
    b = view["vertical"].astype(np.float64)
    c = view["lower_left_corner"].astype(np.float64) - view["origin"].astype(np.float64)
    with np.errstate(all="ignore"):
        ru, rv, rw = _cross(b, c), _cross(c, a), _cross(a, b)
        det = (c[2] * rw[2] + c[1] * rw[1]) + c[0] * rw[0]
        if not np.isfinite(det) or det == 0:
            return None
        if det < 0:
            ru, rv, rw = -ru, -rv, -rw
        return ru.astype(F), rv.astype(F), rw.astype(F), (-1 if det < 0 else 1)


def _dot(r, d):
    return ((r[2] * d[..., 2]).astype(F) + (r[1] * d[..., 1]).astype(F)).astype(F) + (r[0] * d[..., 0]).astype(F)


def reproject(rays, guide, sums, spp, prev_view, prev_guide, prev_hist, max_samples):
    """rays: (H, W, 6) float32 primary rays {origin, direction}; guide: (H, W) guide records (kind, material, plane, t); sums:
    (H, W, 4) float32; prev_view: a view dict or None, with prev_guide (h, w) and prev_hist (h, w, 4) of the earlier frame.
    Returns (hist (H, W, 4), mean (H, W, 4), Q (H, W, 2) int64 — meaningful where on_screen —, found (H, W) bool,
    counts (keyed, found, rejected by key or hn, rejected by nw or off-screen))."""
    rays = np.asarray(rays, F)
    sums = np.asarray(sums, F)
    H, W = guide.shape
    assert rays.shape == (H, W, 6) and sums.shape == (H, W, 4) and spp >= 1
    max_samples = F(max_samples)
    assert max_samples >= 1
    keyed = guide["kind"] != 0
    fspp = F(spp)
    hist = sums.copy()
    hist[..., 3] = fspp
    Q = np.zeros((H, W, 2), np.int64)
    found = np.zeros((H, W), bool)
    counts = [int(keyed.sum()), 0, 0, 0]
    if prev_view is not None:
        ph, pw = prev_guide.shape
        assert prev_hist.shape == (ph, pw, 4) and prev_view["image_width"] >= 2 and prev_view["image_height"] >= 2
        ru, rv, rw, _ = view_rows(prev_view)
        with np.errstate(all="ignore"):
            t = np.ascontiguousarray(guide["t"]).astype(F)[..., None]
            wpt = (rays[..., :3] + (t * rays[..., 3:]).astype(F)).astype(F)
            d = (wpt - prev_view["origin"]).astype(F)
            nu, nv, nw = _dot(ru, d).astype(F), _dot(rv, d).astype(F), _dot(rw, d).astype(F)
            fx = ((nu / nw).astype(F) * F(prev_view["image_width"] - 1)).astype(F)
            fy = ((nv / nw).astype(F) * F(prev_view["image_height"] - 1)).astype(F)
            on_screen = (nw > 0) & (fx >= 0) & (fx < F(pw)) & (fy >= 0) & (fy < F(ph))
            qx = np.where(on_screen, fx, 0).astype(np.int64)
            qy = np.where(on_screen, fy, 0).astype(np.int64)
            Q = np.stack([qx, qy], -1)
            pg = prev_guide[qy, qx]
            same = (pg["kind"] == guide["kind"]) & (pg["material"] == guide["material"]) & \
                (np.ascontiguousarray(pg["plane"]).view(np.uint32) == np.ascontiguousarray(guide["plane"]).view(np.uint32))
            h = np.asarray(prev_hist, F)[qy, qx]
            hn = h[..., 3]
            tried = keyed & on_screen
            found = tried & same & (hn > 0)
            over = hn > max_samples
            s = (max_samples / hn).astype(F)
            rgb = np.where(over[..., None], (h[..., :3] * s[..., None]).astype(F), h[..., :3])
            hn = np.where(over, max_samples, hn)
            hist[..., :3] = np.where(found[..., None], (sums[..., :3] + rgb).astype(F), sums[..., :3])
            hist[..., 3] = np.where(found, (fspp + hn).astype(F), fspp)
        counts[1] = int(found.sum())
        counts[2] = int((tried & ~found).sum())
        counts[3] = int((keyed & ~on_screen).sum())
    with np.errstate(all="ignore"):
        mean = np.ones((H, W, 4), F)
        mean[..., :3] = (hist[..., :3] / hist[..., 3:4]).astype(F)
    return hist, mean, Q, found, tuple(counts)
