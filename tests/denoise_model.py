"""The numpy statement of the guide image and the edge-stopping filter (include/tdt_rt.h, "guide images and the denoiser").

guide_from_hits: the four words of a guide texel from pick's records.  denoise: the a-trous filter in float32 with the tap order
and the operation order the header fixes — j outer, i inner, a multiply and then an add per kept tap, one divide at the end — so
that the GPU's bytes can be compared with it bit for bit.  Skipped taps go through np.where: nothing is ever multiplied by zero
(a NaN or an inf behind a skipped tap must not reach the sum)."""
import numpy as np

GUIDE_DTYPE = np.dtype([("kind", "<u4"), ("material", "<u4"), ("plane", "<f4"), ("t", "<f4")])
B3 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)


def guide_from_hits(hits, materials, all_materials):
    """hits: an array of tdt_ray_hit records (any shape); materials: the slot-1 payload, 3 words per entry (type first).  Returns
    GUIDE_DTYPE records of the same shape."""
    n = hits["normal"]
    s = np.where(n < 0, 0, np.where(n > 0, 2, 1)).astype(np.uint32)
    face = 9 * s[..., 0] + 3 * s[..., 1] + s[..., 2]
    nonzero = n != 0                                                   # (a NaN component counts as non-zero, with s = 1)
    keyed = (hits["status"] == 1) & (hits["fresh_record"] != 0) & nonzero.any(-1)
    if not all_materials:
        words = np.ascontiguousarray(materials).reshape(-1).view(np.uint32)
        first = 3 * hits["material"].astype(np.int64)
        inside = first + 2 < len(words)                                # the whole 12-byte entry lies in the buffer
        typ = np.concatenate([words, np.ones(1, np.uint32)])[np.where(inside, first, len(words))]
        keyed &= inside & (typ == 0)
    a = np.argmax(nonzero, -1)[..., None]                             # the first axis with a non-zero component
    na = np.take_along_axis(n, a, -1)[..., 0]
    ca = np.take_along_axis(hits["cell_min"], a, -1)[..., 0]
    plane = (ca + np.where(na > 0, hits["cell_size"], np.float32(0.0)).astype(np.float32)).astype(np.float32)
    g = np.zeros(hits.shape, GUIDE_DTYPE)
    g["kind"] = np.where(keyed, 1 + face, 0)
    g["material"] = hits["material"]
    g["plane"] = np.where(keyed, plane, np.float32(0.0))
    g["t"] = hits["t"]
    return g


def _keys(guide):
    return np.stack([guide["kind"], guide["material"], np.ascontiguousarray(guide["plane"]).view(np.uint32)], -1)


def _taps(guide, step):
    """For each (j, i) in the contract's order: (j, i, the clipped source rows, columns, and whether the tap is kept), all (H, W)."""
    h, w = guide.shape
    key = _keys(guide)
    ys, xs = np.arange(h), np.arange(w)
    for j in range(-2, 3):
        qy = ys + j * step
        for i in range(-2, 3):
            qx = xs + i * step
            inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
            ry, rx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            kept = inside & (key[np.ix_(ry, rx)] == key).all(-1)
            yield j, i, ry, rx, kept


def kept_taps(guide, step=1):
    """How many taps of a pass of this step each pixel keeps (kind-0 pixels: 0)."""
    n = np.zeros(guide.shape, np.int32)
    for _, _, _, _, kept in _taps(guide, step):
        n += kept
    return np.where(guide["kind"] != 0, n, 0)


def denoise(img, guide, passes):
    """img: (H, W, 4) float32; guide: (H, W) GUIDE_DTYPE; returns the image after `passes` passes (step 2^p in pass p)."""
    img = np.array(img, np.float32, copy=True)
    assert img.shape == guide.shape + (4,) and 0 <= passes <= 8
    filtered = guide["kind"] != 0
    with np.errstate(all="ignore"):
        for p in range(passes):
            num = np.zeros(guide.shape + (3,), np.float32)
            den = np.zeros(guide.shape, np.float32)
            for j, i, ry, rx, kept in _taps(guide, 1 << p):
                wt = np.float32(B3[j + 2] * B3[i + 2])                 # exact in float32
                prod = (wt * img[np.ix_(ry, rx)][..., :3]).astype(np.float32)
                num = np.where(kept[..., None], (num + prod).astype(np.float32), num)
                den = np.where(kept, (den + wt).astype(np.float32), den)
            out = img.copy()
            out[..., :3] = np.where(filtered[..., None], (num / den[..., None]).astype(np.float32), img[..., :3])
            img = out
    return img
