"""Test helper: the whole-depth builds' lookup of a lane *in a band* (csrc/trace_device.hpp band_classify, band_resolve_x) in numpy
float32, beside the level walk it replaces (tree_lookup_pow2's levels: q = fl(v + f) - v, a = q > 0.5, b = q == 1, x index
2v + a + b) and the plain-digit descent the whole-depth table and the parent-index table are filled with.  All functions take arrays
and broadcast them.  Trees are cells payloads as tests/tree_model.py builds them."""
import numpy as np

F = np.float32
BAND = F(2.0) ** F(-11)
FLOOR, PARENT_IDX, WALK = 0, 1, 2               # band_classify's classes


def _nodes(cells):
    return np.asarray(cells, np.uint32).reshape(-1, 2)


def _fetch(nodes, idx):
    """(value, code) of node idx; past the end of the buffer: EMPTY (robust access)."""
    ok = idx < len(nodes)
    at = np.where(ok, idx, 0)
    value = np.where(ok, nodes[at, 0], 0).astype(np.int64)
    typ = np.where(ok, nodes[at, 1], 0)
    return value, np.where(typ == 0, 0, np.where(typ == 2, 2, 1))


def _descend(cells, depth, yi, zi, x_step):
    """The descent with the x index of each level from x_step(level, v) -> (index of the cell half, digit).  Returns levels visited,
    x digits, code and value of the node it ends on, and the cell index held after each level (0 once it has ended)."""
    nodes = _nodes(cells)
    shape = np.broadcast(yi, zi, x_step(1, np.zeros((), np.int64))[0]).shape
    v, alive = np.zeros(shape, np.int64), np.ones(shape, bool)
    m, qx, code, value = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.ones(shape, np.int64), np.zeros(shape, np.int64)
    held = [np.zeros(shape, np.int64)]
    for level in range(1, depth + 1):
        sh = depth - level
        ix, digit = x_step(level, v)
        idx = ix * 4 + ((yi >> sh) & 1) * 2 + ((zi >> sh) & 1)
        val, cd = _fetch(nodes, idx)
        m, qx = np.where(alive, level, m), np.where(alive, 2 * qx + digit, qx)
        code, value = np.where(alive, cd, code), np.where(alive, val, value)
        alive = alive & (cd == 1)
        v = np.where(alive, val, 0)
        held.append(v)
    return m, qx, code, value, held


def walk(cells, depth, fx0, yi, zi):
    """The level walk of a point with x coordinate fx0 in [0, 1) (float32) and finest-level digits yi, zi."""
    fx0 = np.asarray(fx0, F)

    def step(level, v):
        f = fx0 if level == 1 else (lambda t: (t - np.floor(t)).astype(F))(fx0 * F(1 << (level - 1)))
        fv = v.astype(F)
        q = ((fv + f).astype(F) - fv).astype(F)
        a, b = q > F(0.5), q == F(1.0)
        return 2 * v + a + b, (a & ~b).astype(np.int64)
    return _descend(cells, depth, np.asarray(yi, np.int64), np.asarray(zi, np.int64), step)[:4]


def plain(cells, depth, xg, yi, zi):
    """The plain-digit descent of table position (xg, yi, zi); also the cell index held after each level."""
    xg = np.asarray(xg, np.int64)

    def step(level, v):
        d = (xg >> (depth - level)) & 1
        return 2 * v + d, d
    return _descend(cells, depth, np.asarray(yi, np.int64), np.asarray(zi, np.int64), step)


def in_band(fx0, depth):
    tg = np.asarray(fx0, F) * F(1 << depth)
    return ~(np.abs(tg - np.rint(tg)) > BAND)


def classify(fx0, depth):
    """band_classify for lanes in a band: (class, n)."""
    tg = np.asarray(fx0, F) * F(1 << depth)
    rn = np.rint(tg)
    n = rn.astype(np.int64)
    kind = np.where(tg > rn, np.where(n != 0, PARENT_IDX, FLOOR), np.where((tg < rn) & (n & 1 == 1), FLOOR, WALK))
    return kind, n


def trailing_zeros(n):
    n = np.asarray(n, np.int64)
    return np.where(n == 0, 0, np.log2((n & -n).astype(np.float64))).astype(np.int64)


def resolve(cells, depth, fx0, yi, zi):
    """(class, n, resolved table position or -1 for a lane of the walk, a): a = the critical level's decision of the lanes that
    needed the parent's index (else -1)."""
    fx0, yi, zi = np.asarray(fx0, F), np.asarray(yi, np.int64), np.asarray(zi, np.int64)
    kind, n = classify(fx0, depth)
    tg = fx0 * F(1 << depth)
    j = trailing_zeros(np.where(kind == PARENT_IDX, n, 1))
    levels = depth - 1 - j                            # lc - 1
    held = plain(cells, depth, np.where(kind == PARENT_IDX, n, 0), yi, zi)[4]
    v = np.choose(np.clip(levels, 0, depth - 1), held[:depth])
    t = (fx0 * np.exp2(levels).astype(F)).astype(F)
    f = (t - np.floor(t)).astype(F)
    fv = v.astype(F)
    q = ((fv + f).astype(F) - fv).astype(F)
    a = q > F(0.5)
    xg = np.where(kind == PARENT_IDX, np.where(a, n, n - (1 << j)), tg.astype(np.int64))
    return kind, n, np.where(kind == WALK, -1, xg), np.where(kind == PARENT_IDX, a.astype(np.int64), -1)


def band_floats(depth, n):
    """Every float32 in [0, 1) whose 2^depth multiple lies within the band of the integer n >= 1, the centre included."""
    two_d = F(1 << depth)
    c = int(np.array(F(n) / two_d, F).view(np.uint32))
    span = 1 << 15                                # more than the 2^14 floats a side can hold
    bits = np.arange(c - span, c + span + 1, dtype=np.int64)
    bits = bits[(bits > 0) & (bits < 0x3F800000)]
    x = bits.astype(np.uint32).view(F)
    x = x[np.abs(x * two_d - F(n)) <= BAND]
    assert x[0] > bits[0].astype(np.uint32).view(F) or bits[0] == 1
    return x
