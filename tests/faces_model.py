"""The numpy model of the face tools (include/tdt_rt.h tdt_octree_face_regions / tdt_octree_extract_faces /
tdt_octree_edit_faces), the yardstick of the GPU tests, written from the definition: exposure from surface_model.exposed, the face
list as explicit records sorted by (f, w, u, v), adjacency as index pairs found by np.searchsorted on the records' keys, regions by
connect_model.root_of, columns step by step over the selected faces, and the last-wins list.  numpy only."""
import numpy as np

import connect_model as cm
import surface_model as sm
from test_gpu_region_edit import apply_op, morton
from tdt4230_project_raytracing_amd import rt

MATCH_ANY, MATCH_MATERIAL = 0, 1
DISTANCE_MAX = 1023
COLUMNS, TREE = 0, 1
F_, W_, U_, V_, M_, OWNER_ = range(6)          # the columns of a face record


def face_list(V, depth, regions=None):
    """F as (n, 6) int64 records {f, w, u, v, carried material, index of the owner in V}, ordered by f, then w, u, v."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    E = sm.exposed(V, depth, regions)
    out = []
    for f in range(6):
        a, _, u, v = sm.axes(f)
        idx = np.flatnonzero(E[:, f])
        S = V[idx].astype(np.int64)
        rec = np.stack([np.full(len(idx), f, np.int64), S[:, a], S[:, u], S[:, v], S[:, 3], idx.astype(np.int64)], 1)
        out.append(rec[np.lexsort((rec[:, V_], rec[:, U_], rec[:, W_]))])
    return np.concatenate(out)


def quads(F):
    """F as the (n, 8) int32 tdt_quad rows of tdt_octree_extract_surface(merge = 0, by_material = 1)."""
    out = [sm._rows(f, F[F[:, F_] == f, W_], F[F[:, F_] == f, U_], F[F[:, F_] == f, V_], 1, 1, F[F[:, F_] == f, M_]) for f in range(6)]
    return np.ascontiguousarray(np.concatenate(out))


def record_keys(F):
    return (F[:, F_] << 30) | (F[:, W_] << 20) | (F[:, U_] << 10) | F[:, V_]


def half_offsets(connectivity):
    """The positive half of the in-plane neighbour offsets (du, dv): 2 of 4, 4 of 8."""
    return [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])


def edges(F, depth, connectivity, match):
    """(a, b) index pairs of adjacent faces of F, each unordered pair once."""
    n, N = len(F), 1 << depth
    keys = record_keys(F)
    aa, bb = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for du, dv in half_offsets(connectivity):
        qu, qv = F[:, U_] + du, F[:, V_] + dv
        idx = np.flatnonzero((qu >= 0) & (qu < N) & (qv >= 0) & (qv < N))     # nothing wraps around the grid
        if not len(idx):
            continue
        kq = (F[idx, F_] << 30) | (F[idx, W_] << 20) | (qu[idx] << 10) | qv[idx]
        j = np.minimum(np.searchsorted(keys, kq), n - 1)
        found = keys[j] == kq
        a, b = idx[found], j[found]
        if match == MATCH_MATERIAL:
            same = F[a, M_] == F[b, M_]
            a, b = a[same], b[same]
        aa.append(a)
        bb.append(b)
    return np.concatenate(aa), np.concatenate(bb)


def face_regions(F, depth, connectivity=4, match=MATCH_MATERIAL):
    """(labels uint32, table of rt.FACE_REGION_DTYPE) as tdt_octree_face_regions defines them."""
    n = len(F)
    a, b = edges(F, depth, connectivity, match)
    root = cm.root_of(n, a, b)
    roots = np.flatnonzero(root == np.arange(n))
    labels = np.searchsorted(roots, root)
    tab = np.zeros(len(roots), rt.FACE_REGION_DTYPE)
    tab["first"] = roots
    tab["faces"] = np.bincount(labels, minlength=len(roots))
    if n:
        tab["face"], tab["w"], tab["material"] = F[roots, F_], F[roots, W_], F[roots, M_]
        order = np.argsort(labels, kind="stable")
        starts = np.searchsorted(labels[order], np.arange(len(roots)))
        for k, col in enumerate((U_, V_)):
            c = F[order, col]
            tab["lo"][:, k] = np.minimum.reduceat(c, starts)
            tab["hi"][:, k] = np.maximum.reduceat(c, starts)
    return labels.astype(np.uint32), tab


def selected(F, labels, n_regions, seeds):
    """A bool per region: one of the seeds {x, y, z, f} names one of its faces."""
    sel = np.zeros(n_regions, bool)
    s = np.asarray(seeds, np.int64).reshape(-1, 4)
    if not len(s) or not len(F):
        return sel
    assert ((s[:, 3] >= 0) & (s[:, 3] <= 5)).all(), "a seed's face must be 0..5"
    a = s[:, 3] >> 1
    rows = np.arange(len(s))
    w, u, v = s[rows, a], s[rows, (a + 1) % 3], s[rows, (a + 2) % 3]
    ok = ((s[:, :3] >= 0) & (s[:, :3] < 1024)).all(1)                        # (a seed off the grid is no face of F either way)
    keys = record_keys(F)
    kq = ((s[:, 3] << 30) | (w << 20) | (u << 10) | v)[ok]
    j = np.minimum(np.searchsorted(keys, kq), len(F) - 1)
    sel[labels[j[keys[j] == kq]]] = True
    return sel


def column_pairs(V, F, member, depth, distance, block, material):
    """The (voxel, material) pairs of the columns of the faces F[member], in the order of F, then k: (n, 4) int64 {x, y, z, m}."""
    V = np.asarray(V, np.int64).reshape(-1, 4)
    N = 1 << depth
    idx = np.flatnonzero(member)
    if distance == 0 or not len(idx):
        return np.zeros((0, 4), np.int64)
    kv = np.sort(morton(V[:, :3]))
    S = F[idx]
    a = S[:, F_] >> 1
    normal = np.zeros((len(S), 3), np.int64)
    normal[np.arange(len(S)), a] = np.where(S[:, F_] & 1, 1, -1)
    owner = V[S[:, OWNER_], :3]
    m = S[:, M_] if material < 0 else np.full(len(S), material + 1, np.int64)
    alive = np.ones(len(S), bool)
    chunks = []
    for t in range(abs(distance)):
        q = owner + normal * (t + 1) if distance > 0 else owner - normal * t
        alive &= ((q >= 0) & (q < N)).all(1)
        if block:
            solid = np.zeros(len(S), bool)
            solid[alive] = np.isin(morton(q[alive]), kv)
            alive &= ~solid if distance > 0 else solid
        if not alive.any():
            break
        rows = np.flatnonzero(alive)
        chunks.append(np.concatenate([rows[:, None], np.full((len(rows), 1), t), q[rows], m[rows, None]], 1))
    if not chunks:
        return np.zeros((0, 4), np.int64)
    P = np.concatenate(chunks)
    return P[np.lexsort((P[:, 1], P[:, 0]))][:, 2:]


def last_wins(P):
    """A pair list reduced by the builder's rule — of duplicates the last one wins — Morton-sorted: (n, 4) int32."""
    P = np.asarray(P, np.int64).reshape(-1, 4)
    key = morton(P[:, :3])
    order = np.argsort(key, kind="stable")
    key = key[order]
    last = np.ones(len(key), bool)
    last[:-1] = key[1:] != key[:-1]
    return np.ascontiguousarray(P[order][last].astype(np.int32))


def column_list(V, depth, seeds, distance, connectivity=4, match=MATCH_MATERIAL, block=False, material=-1, regions=None):
    """What tdt_octree_extract_faces(TDT_FACES_COLUMNS) returns."""
    assert abs(distance) <= DISTANCE_MAX and -1 <= material <= 253
    F = face_list(V, depth, regions)
    labels, tab = face_regions(F, depth, connectivity, match)
    member = selected(F, labels, len(tab), seeds)[labels] if len(F) else np.zeros(0, bool)
    return last_wins(column_pairs(V, F, member, depth, distance, bool(block), material))


def intersect(V, B):
    """V's voxels that B holds, with V's materials."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    return np.ascontiguousarray(V[np.isin(morton(V[:, :3]), morton(np.asarray(B).reshape(-1, 4)[:, :3]))])


def extract(V, depth, seeds, distance, what=COLUMNS, **kw):
    """What tdt_octree_extract_faces returns."""
    B = column_list(V, depth, seeds, distance, **kw)
    return B if what == COLUMNS else intersect(V, B)


def edit(V, depth, op, seeds, distance, **kw):
    """The voxel list tdt_octree_edit_faces leaves, Morton-sorted."""
    return apply_op(V, op, column_list(V, depth, seeds, distance, **kw), 0)
