"""numpy model of tdt_image_upsample: the lines of include/tdt_rt.h restated, every operation in float32 and rounded on its own, so
that the GPU's bytes can be compared bit for bit.  Also the hand-made cases the GPU test runs, so that the CPU test can assert what
they reach (tests/test_upsample_model.py, tests/test_gpu_upsample.py)."""
import numpy as np

from denoise_model import GUIDE_DTYPE

F = np.float32


def axis_map(W, w):
    """(i0, i1, nearest, f) of every pixel 0..W-1 of a side of W pixels over a side of w texels, exact integers and one divide."""
    x = np.arange(W, dtype=np.int64)
    if W == 1:
        i0, r, f = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, F)
    else:
        n = x * (w - 1)
        i0, r = n // (W - 1), n % (W - 1)
        f = r.astype(F) / F(W - 1)
    i1 = np.minimum(i0 + 1, w - 1)
    return i0, i1, np.where(2 * r < W - 1, i0, i1), f


def _key(guide):
    """(H, W, 3) uint32: words 0, 1, 2 of a guide given as GUIDE_DTYPE records or as (H, W, 4) words / floats."""
    g = np.ascontiguousarray(guide)
    h, w = g.shape[:2]
    return g.view(np.uint32).reshape(h, w, 4)[..., :3]


def upsample(dst_guide, src, src_guide, with_skipped=False):
    """src: (h, w, 4) float32; the guides: (H, W) and (h, w).  Returns (image (H, W, 4) float32, class map (H, W) of 1, 2, 3), and
    with_skipped also the mask of the pixels where stage 1 skipped a tap of positive weight for its key — the edge pixels."""
    gk, sk = _key(dst_guide), _key(src_guide)
    src = np.ascontiguousarray(src, F)
    H, W = gk.shape[:2]
    h, w = sk.shape[:2]
    assert src.shape == (h, w, 4) and 1 <= w <= W and 1 <= h <= H
    i0, i1, i_near, fx = axis_map(W, w)
    j0, j1, j_near, fy = axis_map(H, h)
    wx, wy = (F(1.0) - fx, fx), (F(1.0) - fy, fy)
    num, den = np.zeros((H, W, 4), F), np.zeros((H, W), F)
    skipped = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for b, jj in enumerate((j0, j1)):
            for a, ii in enumerate((i0, i1)):
                wt = wy[b][:, None] * wx[a][None, :]
                same = (sk[jj[:, None], ii[None, :]] == gk).all(-1)
                keep = (wt > 0) & same
                skipped |= (wt > 0) & ~same
                c = src[jj[:, None], ii[None, :]]
                num = np.where(keep[..., None], num + wt[..., None] * c, num)
                den = np.where(keep, den + wt, den)
        cls = np.where(den > 0, 1, 0)
        out = np.where((cls == 1)[..., None], num / np.where(den > 0, den, F(1))[..., None], F(0)).astype(F)
        ring = cls == 0                                                   # (num is still zero there)
        K = np.zeros((H, W), F)
        for dj in range(-1, 3):
            for di in range(-1, 3):
                qy, qx = (j0 + dj)[:, None], (i0 + di)[None, :]
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                cy, cx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                keep = ring & inside & (sk[cy, cx] == gk).all(-1)
                num = np.where(keep[..., None], num + src[cy, cx], num)
                K = np.where(keep, K + F(1.0), K)
        two = ring & (K > 0)
        out = np.where(two[..., None], num / np.where(K > 0, K, F(1))[..., None], out).astype(F)
    cls = np.where(two, 2, cls)
    hole = cls == 0
    nearest = src[j_near[:, None], i_near[None, :]]
    out_bits = np.where(hole[..., None], nearest.view(np.uint32), out.view(np.uint32))      # (bit for bit: no arithmetic touches it)
    cls = np.where(hole, 3, cls)
    out = np.ascontiguousarray(out_bits).view(F)
    return (out, cls, skipped) if with_skipped else (out, cls)


def histogram(cls):
    """What tdt_debug_upsample_counts reports for a class map."""
    return (int(cls.size), int((cls == 1).sum()), int((cls == 2).sum()), int((cls == 3).sum()))


# ---- the hand-made cases: (W, H, w, h, seed) ----
HAND_CASES = [(1, 1, 1, 1, 1), (2, 2, 1, 1, 3), (17, 16, 9, 8, 3), (33, 17, 17, 9, 4), (33, 17, 16, 8, 5), (7, 5, 2, 5, 6),
              (50, 50, 17, 17, 7), (64, 48, 64, 48, 8), (4097, 2, 1366, 2, 9), (32768, 1, 32767, 1, 10)]
MULTI_CASE = (33, 17, 16, 8, 11)                     # the multi-device and the error tests' data


def make_case(W, H, w, h, seed):
    """Guides whose texels are drawn one by one from a small alphabet of keys — two of them kind 0 (sky, and a pass-through hit of
    material 3), one an ulp of `plane` from another, one differing only in material — with a twelfth of the full-resolution
    pixels carrying a key of their own that no source texel has (holes); a source with negatives, -0, denormals, infinities of ONE
    sign per case and NaNs of one payload (inf - inf and an operation on two different NaNs leave sign and payload to the
    implementation).  Returns (dst_guide, src, src_guide)."""
    rng = np.random.default_rng(seed)
    base = F(0.3125)
    keys = [(14, 2, base), (14, 2, np.nextafter(base, F(1))), (14, 3, base), (0, 0, F(0)), (0, 3, F(0))]

    def guide_of(gw, gh, p):
        g = np.zeros((gh, gw), GUIDE_DTYPE)
        which = rng.choice(len(keys), size=(gh, gw), p=p)
        for f, col in (("kind", 0), ("material", 1), ("plane", 2)):
            g[f] = np.array([k[col] for k in keys])[which]
        g["t"] = (0.3 + 2.7 * rng.random((gh, gw))).astype(F)
        return g
    dst_guide = guide_of(W, H, [0.3, 0.2, 0.2, 0.2, 0.1])
    src_guide = guide_of(w, h, [0.25, 0.25, 0.2, 0.2, 0.1])
    flat = dst_guide.reshape(-1)
    for k, p in enumerate(rng.permutation(W * H)[:W * H // 12]):
        flat[p] = (20, 100 + k, F(k), flat[p]["t"])
    c = (rng.standard_normal((h, w, 4)) * 3).astype(F)
    special = rng.random((h, w, 4))
    c[special < 0.04] = F(1e-41)
    c[(special >= 0.04) & (special < 0.06)] = F(-3e-42)
    c[(special >= 0.06) & (special < 0.07)] = F(np.inf if seed % 2 else -np.inf)
    c[(special >= 0.07) & (special < 0.08)] = F(np.nan)
    c[(special >= 0.08) & (special < 0.11)] = F(-0.0)
    return dst_guide, c, src_guide
