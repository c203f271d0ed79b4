"""The numpy statement of adaptive sampling (include/tdt_rt.h, tdt_dispatch_accumulate_masked and "adaptive sampling: the sampling
controller"): which texels of a mask are live, tdt_image_adapt, its counts and tdt_image_adapt_mean in float32, every operation
rounded on its own and in the order the header fixes, so that the GPU's bytes can be compared with them bit for bit; and the frame
Renderer.render_adaptive makes, run over the CPU oracle.  lum is variance_model's, the key comparison denoise_model's.  Where a line
computes a NaN the header leaves its sign and payload open, and the GPU tests compare such values as NaNs."""
import numpy as np

import denoise_model
from variance_model import lum

F = np.float32


def live(mask):
    """mask (H, W, 4): w >= 0.  +0 and -0 are live, negative values and NaN are not."""
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, F)[..., 3] >= F(0)


def _update(sums, state_in, k, tolerance, floor, min_samples, max_samples):
    """The header's update of every texel: (the state after the batch with w still positive, stopped before, capped, passes)."""
    st = np.asarray(state_in, F)
    kf, lo, hi = F(k), F(min_samples), F(max_samples)
    tolerance, floor = F(tolerance), F(floor)
    stopped = ~live(st)
    with np.errstate(all="ignore"):
        Lc = lum(np.asarray(sums, F)[..., :3])
        lb = ((Lc - st[..., 0]).astype(F) / kf).astype(F)
        m2 = (st[..., 1] + (lb * lb).astype(F)).astype(F)
        n = (st[..., 2] + F(1)).astype(F)
        s = (st[..., 3] + kf).astype(F)
        mean = (Lc / s).astype(F)
        v = ((m2 / n).astype(F) - (mean * mean).astype(F)).astype(F)
        var = np.where(v < 0, F(0), v)                                    # (a NaN stays a NaN)
        err2 = (var / n).astype(F)
        mx = np.where(mean > floor, mean, floor)
        thr = (tolerance * mx).astype(F)
        thr2 = (thr * thr).astype(F)
        capped = ~stopped & (s >= hi)
        own = (s >= lo) & (n >= F(2)) & (err2 <= thr2)
    passes = stopped | capped | own
    return np.stack([Lc, m2, n, s], -1).astype(F), stopped, capped, passes


def adapt(sums, guide, state_in, k, tolerance, floor, min_samples, max_samples):
    """tdt_image_adapt: (state_out (H, W, 4), counts (live before, stopped by the tolerance, by the cap, still live)).  guide: None
    or (H, W) GUIDE_DTYPE records."""
    st = np.ascontiguousarray(state_in, F)
    h, w = st.shape[:2]
    new, stopped, capped, passes = _update(sums, st, k, tolerance, floor, min_samples, max_samples)
    stop = passes.copy()
    if guide is not None:
        key = denoise_model._keys(guide)
        ys, xs = np.arange(h), np.arange(w)
        for j in (-1, 0, 1):
            qy = ys + j
            for i in (-1, 0, 1):
                qx = xs + i
                inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
                ry, rx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                same = inside & (key[np.ix_(ry, rx)] == key).all(-1)
                stop &= ~(same & ~passes[np.ix_(ry, rx)])
        stop |= capped
    out = new.copy()
    with np.errstate(all="ignore"):
        out[..., 3] = np.where(stop, -new[..., 3], new[..., 3])
    out_bits = np.where(stopped[..., None], st.view(np.uint32), out.view(np.uint32))      # (a stopped pixel: bit for bit)
    alive = ~stopped
    counts = (int(alive.sum()), int((alive & stop & ~capped).sum()), int((alive & capped).sum()), int((alive & ~stop).sum()))
    return np.ascontiguousarray(out_bits).view(F), counts


def adapt_mean(img, state):
    """tdt_image_adapt_mean: rgb / |w|, alpha = the variance of the mean luminance; texels with |w| == 0 are left alone."""
    img, st = np.ascontiguousarray(img, F), np.asarray(state, F)
    with np.errstate(all="ignore"):
        aw = np.abs(st[..., 3])
        n = st[..., 2]
        mean = (st[..., 0] / aw).astype(F)
        v = ((st[..., 1] / n).astype(F) - (mean * mean).astype(F)).astype(F)
        v = np.where(v > 0, v, F(0))
        a = np.where(n >= F(2), (v / n).astype(F), F(0))
        out = np.concatenate([(img[..., :3] / aw[..., None]).astype(F), a[..., None].astype(F)], -1)
    out_bits = np.where((aw == 0)[..., None], img.view(np.uint32), np.ascontiguousarray(out).view(np.uint32))
    return np.ascontiguousarray(out_bits).view(F)


def masked_accumulate(oracle, scene, cam, accum, carry, begin, count, mask, dispatch=None, threads=16):
    """tdt_dispatch_accumulate_masked over the oracle, in place: everything is traced into a copy, and the live pixels' image texel
    and carry are kept.  (Pixels the dispatch does not cover come back unchanged from the oracle, so keeping them changes nothing.)"""
    a, c = accum.copy(), (carry.copy() if carry is not None else None)
    oracle.accumulate(scene, cam, a, c, begin, count, dispatch=dispatch, threads=threads)
    m = live(mask)
    accum[m] = a[m]
    if carry is not None:
        carry[m] = c[m]


def render_adaptive(oracle, scene, cam, tolerance, batch=2, min_samples=4, max_samples=None, floor=0.05, guide=None, dispatch=None,
                    threads=16):
    """Renderer.render_adaptive's loop up to the final state: dict(sums, state, samples (H, W) int, rounds, counts per round).
    dispatch: None = (W + 1, H + 1), the renderer's; pixels it does not cover receive nothing and stop at the cap like the others."""
    W, H = cam.image_width, cam.image_height
    cap = cam.samples_per_pixel if max_samples is None else max_samples
    sums, carry, state = np.zeros((H, W, 4), F), np.zeros((H, W, 16), F), np.zeros((H, W, 4), F)
    begin, rounds, history = 0, 0, []
    while True:
        masked_accumulate(oracle, scene, cam, sums, carry, begin, batch, state, dispatch=dispatch, threads=threads)
        state, counts = adapt(sums, guide, state, batch, tolerance, floor, min_samples, cap)
        history.append(counts)
        begin += batch
        rounds += 1
        if counts[3] == 0:
            break
    return {"sums": sums, "state": state, "samples": np.abs(state[..., 3]).astype(np.int64), "rounds": rounds, "counts": history}


def make_case(w, h, seed, with_guide=True, specials=True):
    """Hand-made (sums, guide, state_in) of one size: faces a few pixels wide whose edges cross the 32x8 tile borders, states with
    zero, one and several batches behind them, stopped pixels, and (specials) NaN, infinities, denormals and -0 in sums and state."""
    rng = np.random.default_rng(seed)
    guide = None
    if with_guide:
        guide = np.zeros((h, w), denoise_model.GUIDE_DTYPE)
        ys, xs = np.mgrid[0:h, 0:w]
        face = ((xs + 3) // 7 + 5 * ((ys + 2) // 6)) % 11                   # (edges at x = 4, 11, .., 32 - 4, ..: not the tiles')
        guide["kind"] = np.where(face == 0, 0, 1 + face % 5)
        guide["material"] = face // 2
        guide["plane"] = (face % 3).astype(F)
        guide["t"] = rng.random((h, w), dtype=F)                          # (not part of the key)
    nb = rng.integers(0, 5, (h, w))                                       # batches behind the pixel
    k = 2
    s = (nb * k).astype(F)
    base = rng.random((h, w, 3), dtype=F) * F(2)
    noise = np.where(rng.random((h, w, 1)) < 0.5, F(0.02), F(0.6))        # quiet and noisy pixels side by side
    sums = np.zeros((h, w, 4), F)
    sums[..., :3] = (base * (s[..., None] + k) + noise * rng.standard_normal((h, w, 3)).astype(F)).astype(F)
    state = np.zeros((h, w, 4), F)
    state[..., 0] = lum((base * s[..., None]).astype(F))
    state[..., 1] = (nb * lum(base) ** 2 * (1 + 0.1 * rng.random((h, w)))).astype(F)
    state[..., 2] = nb
    state[..., 3] = np.where(rng.random((h, w)) < 0.2, -s, s)             # one in five has stopped (w = -0 with no batches: live)
    if specials and w * h >= 64:
        flat_s, flat_t = sums.reshape(-1, 4), state.reshape(-1, 4)
        idx = rng.choice(w * h, 24, replace=False)
        vals = [np.nan, np.inf, -np.inf, 1e-42, -0.0, 3e38]
        for n, p in enumerate(idx[:12]):
            flat_s[p, n % 3] = vals[n % 6]
        for n, p in enumerate(idx[12:]):
            flat_t[p, n % 4] = vals[n % 6]
    return sums, guide, state


SIZES = [(1, 1), (2, 2), (33, 17), (257, 19), (19, 257)]
# (tolerance, floor, min_samples, max_samples) around the sample counts make_case produces (0, 2, .., 8 before the batch of 2)
LIMITS = [(0.05, 0.05, 4, 64), (0.5, 0.0, 0, 64), (0.05, 0.05, 6, 6), (0.2, 0.1, 10, 8), (0.0, 0.0, 4, 1 << 24)]
