"""The numpy statement of the luminance variance and the variance-guided filter (include/tdt_rt.h, "luminance variance and the
variance-guided filter"): variance, denoise_variance and reproject_moments in float32, every operation rounded on its own and in
the order the header fixes, so that the GPU's bytes can be compared with them bit for bit.  Skipped taps go through np.where, as in
denoise_model.py: nothing is multiplied by zero.  The guide's record type and the key comparison are denoise_model's, the
projection is reproject_model's; neither is restated here."""
import numpy as np

import denoise_model
import reproject_model
from denoise_model import B3, GUIDE_DTYPE  # noqa: F401

F = np.float32
G3 = np.array([1 / 4, 1 / 2, 1 / 4], F)


def lum(rgb):
    """(0.2126 r + 0.7152 g) + 0.0722 b over the last axis, three multiplies and two adds."""
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        return ((F(0.2126) * rgb[..., 0]).astype(F) + (F(0.7152) * rgb[..., 1]).astype(F)).astype(F) + (F(0.0722) * rgb[..., 2]).astype(F)


def _window(guide, radius, step=1):
    """For each (j, i) of a (2 radius + 1)^2 window in the contract's order: (j, i, clipped rows, columns, kept), as denoise_model._taps."""
    h, w = guide.shape
    key = denoise_model._keys(guide)
    ys, xs = np.arange(h), np.arange(w)
    for j in range(-radius, radius + 1):
        qy = ys + j * step
        for i in range(-radius, radius + 1):
            qx = xs + i * step
            inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
            ry, rx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            yield j, i, ry, rx, inside & (key[np.ix_(ry, rx)] == key).all(-1)


def variance(img, guide, moments=None, min_frames=4.0):
    """img (H, W, 4) with alpha replaced by the variance of the luminance of rgb: 0 where kind == 0, the temporal estimate where
    moments (H, W, 4) = (m1, m2, n, 0) has n >= min_frames, the 7x7 same-key estimate elsewhere."""
    img = np.array(img, F, copy=True)
    assert img.shape == guide.shape + (4,)
    min_frames = F(min_frames)
    assert min_frames >= 1
    with np.errstate(all="ignore"):
        l = lum(img[..., :3])
        K = np.zeros(guide.shape, F)
        s1 = np.zeros(guide.shape, F)
        s2 = np.zeros(guide.shape, F)
        for _, _, ry, rx, kept in _window(guide, 3):
            lq = l[np.ix_(ry, rx)]
            K = np.where(kept, (K + F(1)).astype(F), K)
            s1 = np.where(kept, (s1 + lq).astype(F), s1)
            s2 = np.where(kept, (s2 + (lq * lq).astype(F)).astype(F), s2)
        mu = (s1 / K).astype(F)
        v = ((s2 / K).astype(F) - (mu * mu).astype(F)).astype(F)
        a = np.where(v > 0, v, F(0))
        if moments is not None:
            m = np.asarray(moments, F)
            assert m.shape == img.shape
            n = m[..., 2]
            mu = (m[..., 0] / n).astype(F)
            e2 = (m[..., 1] / n).astype(F)
            v = (e2 - (mu * mu).astype(F)).astype(F)
            v = np.where(v > 0, v, F(0))
            a = np.where(n >= min_frames, (v / n).astype(F), a)
        img[..., 3] = np.where(guide["kind"] != 0, a, F(0))
    return img


def classify(img, guide, step, sigma, floor=0.0):
    """What one pass of this step does with the taps, from the model alone: (copied (H, W): kind != 0 and lim not in (0, inf);
    kept (H, W): how many same-key taps of a filtered pixel, the centre included, the luminance weight keeps; rejected (H, W): how
    many it drops)."""
    _, copied, kept, rejected = _pass(np.asarray(img, F), guide, step, (F(sigma) * F(sigma)).astype(F), F(floor))
    return copied, kept, rejected


def _pass(img, guide, step, s2, floor):
    filtered = guide["kind"] != 0
    with np.errstate(all="ignore"):
        l = lum(img[..., :3])
        gnum = np.zeros(guide.shape, F)
        gden = np.zeros(guide.shape, F)
        for j, i, ry, rx, kept in _window(guide, 1):
            wg = F(G3[j + 1] * G3[i + 1])
            gnum = np.where(kept, (gnum + (wg * img[np.ix_(ry, rx)][..., 3]).astype(F)).astype(F), gnum)
            gden = np.where(kept, (gden + wg).astype(F), gden)
        gv = (gnum / gden).astype(F)
        lim = ((s2 * gv).astype(F) + floor).astype(F)
        active = filtered & (lim > 0) & (lim < F(np.inf))
        num = np.zeros(guide.shape + (3,), F)
        den = np.zeros(guide.shape, F)
        vnum = np.zeros(guide.shape, F)
        n_kept = np.zeros(guide.shape, np.int32)
        n_rejected = np.zeros(guide.shape, np.int32)
        for j, i, ry, rx, same in _window(guide, 2, step):
            q = img[np.ix_(ry, rx)]
            d = (l[np.ix_(ry, rx)] - l).astype(F)
            d2 = (d * d).astype(F)
            kept = same & (d2 < lim)
            n_kept += kept & active
            n_rejected += same & ~kept & active
            wt = (F(B3[j + 2] * B3[i + 2]) * (lim - d2).astype(F)).astype(F)
            num = np.where(kept[..., None], (num + (wt[..., None] * q[..., :3]).astype(F)).astype(F), num)
            den = np.where(kept, (den + wt).astype(F), den)
            vnum = np.where(kept, (vnum + ((wt * wt).astype(F) * q[..., 3]).astype(F)).astype(F), vnum)
        out = img.copy()
        out[..., :3] = np.where(active[..., None], (num / den[..., None]).astype(F), img[..., :3])
        out[..., 3] = np.where(active, (vnum / (den * den).astype(F)).astype(F), img[..., 3])
    return out, filtered & ~active, n_kept, n_rejected


def denoise_variance(img, guide, passes, sigma, floor=0.0):
    """img: (H, W, 4) float32 whose alpha is the variance of its luminance; returns the image after `passes` passes."""
    img = np.array(img, F, copy=True)
    assert img.shape == guide.shape + (4,) and 0 <= passes <= 8
    sigma, floor = F(sigma), F(floor)
    assert sigma > 0 and np.isfinite(sigma) and floor >= 0 and np.isfinite(floor)
    s2 = (sigma * sigma).astype(F)
    for p in range(passes):
        img = _pass(img, guide, 1 << p, s2, floor)[0]
    return img


def reproject_moments(rays, guide, sums, spp, prev_view, prev_guide, prev_hist, prev_moments, max_samples):
    """reproject_model.reproject's (hist, mean, Q, found, counts) and, before them, the moments image (H, W, 4) = (m1, m2, n, 0)."""
    hist, mean, Q, found, counts = reproject_model.reproject(rays, guide, sums, spp, prev_view, prev_guide, prev_hist, max_samples)
    sums = np.asarray(sums, F)
    with np.errstate(all="ignore"):
        l = lum((sums[..., :3] / F(spp)).astype(F))
        ll = (l * l).astype(F)
        out = np.zeros(sums.shape, F)
        out[..., 0], out[..., 1], out[..., 2] = l, ll, F(1)
        if prev_view is not None:
            hm = np.asarray(prev_moments, F)[Q[..., 1], Q[..., 0]]
            assert hm.shape == sums.shape
            mf = (F(max_samples) / F(spp)).astype(F)
            n = hm[..., 2]
            use = found & (n > 0)
            over = n > mf
            sc = (mf / n).astype(F)
            m1 = np.where(over, (hm[..., 0] * sc).astype(F), hm[..., 0])
            m2 = np.where(over, (hm[..., 1] * sc).astype(F), hm[..., 1])
            n = np.where(over, mf, n)
            out[..., 0] = np.where(use, (l + m1).astype(F), l)
            out[..., 1] = np.where(use, (ll + m2).astype(F), ll)
            out[..., 2] = np.where(use, (F(1) + n).astype(F), F(1))
    return out, hist, mean, Q, found, counts
