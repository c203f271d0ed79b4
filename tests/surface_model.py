"""The numpy model of surface extraction (include/tdt_rt.h tdt_octree_extract_surface) and of tdt_quads_to_mesh
(include/tdt_host.h), the yardstick of the GPU tests, written from the definition: a dense padded occupancy array, a lexsort per
face direction, runs and then stacks.  `quads_loop` walks the sorted faces and runs one by one in Python; `quads` finds the same
heads with array comparisons (the GPU suites' larger trees need it) and tests/test_surface_api.py pins the two to each other.
numpy only."""
import numpy as np

import fill_model as fm
from test_gpu_region_edit import inside
from tdt4230_project_raytracing_amd import rt

UNIT = 64
DENSE_DEPTH = 9                # above it the occupancy test is a search in sorted linear indices (a depth-10 grid has 2^30 voxels)


def axes(f):
    """(a, s, u, v) of face f."""
    a = f >> 1
    return a, f & 1, (a + 1) % 3, (a + 2) % 3


def exposed(V, depth, regions=None):
    """(len(V), 6) bool: face f of voxel i is exposed and voxel i is inside the mask (regions None: no mask)."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    n = 1 << depth
    p = V[:, :3].astype(np.int64)
    out = np.zeros((len(V), 6), bool)
    if depth <= DENSE_DEPTH:
        occ = np.zeros((n + 2,) * 3, bool)                     # one empty layer all round: outside the grid counts as empty
        occ[p[:, 0] + 1, p[:, 1] + 1, p[:, 2] + 1] = True
    else:
        lin = np.sort((p[:, 0] * n + p[:, 1]) * n + p[:, 2])
    for f in range(6):
        a, s, _, _ = axes(f)
        q = p.copy()
        q[:, a] += 1 if s else -1
        if depth <= DENSE_DEPTH:
            out[:, f] = ~occ[q[:, 0] + 1, q[:, 1] + 1, q[:, 2] + 1]
        else:
            ok = (q[:, a] >= 0) & (q[:, a] < n)
            out[:, f] = ~(ok & np.isin((q[:, 0] * n + q[:, 1]) * n + q[:, 2], lin))
    if regions is not None:
        regions = [regions] if isinstance(regions, rt.Region) else list(regions)
        out &= (inside(V[:, :3], regions) if len(regions) else np.zeros(len(V), bool))[:, None]
    return out


def _faces(V, E, f, by_material):
    """The exposed faces of direction f as (w, u, v, carried material) columns."""
    a, _, u, v = axes(f)
    S = V[E[:, f]].astype(np.int64)
    return S[:, a], S[:, u], S[:, v], (S[:, 3] if by_material else np.zeros(len(S), np.int64))


def _rows(f, w, u0, v0, su, sv, m):
    a, s, u, v = axes(f)
    out = np.zeros((len(w), 8), np.int32)
    out[:, 0], out[:, 1] = f, m
    out[:, 2 + a], out[:, 2 + u], out[:, 2 + v] = w + s, u0, v0
    out[:, 5], out[:, 6] = su, sv
    return out


def quads_loop(V, depth, merge=True, by_material=True, regions=None):
    """The definition, item by item."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    E = exposed(V, depth, regions)
    out = []
    for f in range(6):
        w, u, v, m = _faces(V, E, f, by_material)
        if not merge:
            o = np.lexsort((v, u, w))
            out.append(_rows(f, w[o], u[o], v[o], 1, 1, m[o]))
            continue
        runs = []                                              # [w, v, u0, u1, m]
        for i in np.lexsort((u, v, w)):
            if runs and runs[-1][0] == w[i] and runs[-1][1] == v[i] and runs[-1][3] + 1 == u[i] and runs[-1][4] == m[i]:
                runs[-1][3] = u[i]
            else:
                runs.append([w[i], v[i], u[i], u[i], m[i]])
        stacks = []                                            # [w, u0, u1, m, v0, v1]
        for rw, rv, u0, u1, rm in sorted(runs, key=lambda r: (r[0], r[2], r[1])):
            if stacks and stacks[-1][:4] == [rw, u0, u1, rm] and stacks[-1][5] + 1 == rv:
                stacks[-1][5] = rv
            else:
                stacks.append([rw, u0, u1, rm, rv, rv])
        q = np.array(stacks, np.int64).reshape(-1, 6)
        out.append(_rows(f, q[:, 0], q[:, 1], q[:, 4], q[:, 2] - q[:, 1] + 1, q[:, 5] - q[:, 4] + 1, q[:, 3]))
    return np.ascontiguousarray(np.concatenate(out))


def quads(V, depth, merge=True, by_material=True, regions=None):
    """(n, 8) int32 tdt_quad rows, ordered by face, w, u0, v0."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    E = exposed(V, depth, regions)
    out = []
    for f in range(6):
        w, u, v, m = _faces(V, E, f, by_material)
        if not merge:
            o = np.lexsort((v, u, w))
            out.append(_rows(f, w[o], u[o], v[o], 1, 1, m[o]))
            continue
        o = np.lexsort((u, v, w))
        w, u, v, m = w[o], u[o], v[o], m[o]
        head = np.ones(len(w), bool)
        head[1:] = (w[1:] != w[:-1]) | (v[1:] != v[:-1]) | (u[1:] != u[:-1] + 1) | (m[1:] != m[:-1])
        at = np.flatnonzero(head)
        u1 = u[np.append(at[1:], len(w)) - 1] if len(at) else u[:0]
        w, v, u0, m = w[at], v[at], u[at], m[at]
        o = np.lexsort((v, u0, w))
        w, v, u0, u1, m = w[o], v[o], u0[o], u1[o], m[o]
        head = np.ones(len(w), bool)
        head[1:] = (w[1:] != w[:-1]) | (u0[1:] != u0[:-1]) | (v[1:] != v[:-1] + 1) | (u1[1:] != u1[:-1]) | (m[1:] != m[:-1])
        at = np.flatnonzero(head)
        v1 = v[np.append(at[1:], len(w)) - 1] if len(at) else v[:0]
        out.append(_rows(f, w[at], u0[at], v[at], u1[at] - u0[at] + 1, v1 - v[at] + 1, m[at]))
    return np.ascontiguousarray(np.concatenate(out))


def quads_to_mesh(Q):
    """tdt_quads_to_mesh: (vertices (k, 3) int32 units, welded, ascending (x, y, z); triangles (2 n, 3) uint32; materials (2 n,))."""
    Q = np.asarray(Q, np.int64).reshape(-1, 8)
    corners = np.zeros((len(Q), 4, 3), np.int64)
    for i, q in enumerate(Q):
        _, s, u, v = axes(int(q[0]))
        c = [q[2:5].copy() for _ in range(4)]
        c[1][u] += q[5]
        c[2][u] += q[5]
        c[2][v] += q[6]
        c[3][v] += q[6]
        corners[i] = c if s else [c[0], c[3], c[2], c[1]]
    flat = corners.reshape(-1, 3) * UNIT
    if not len(flat):
        return np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), np.zeros(0, np.int32)
    verts, inv = np.unique(flat, axis=0, return_inverse=True)      # rows in ascending (x, y, z) order
    inv = inv.reshape(-1, 4)
    tris = np.stack([inv[:, [0, 1, 2]], inv[:, [0, 2, 3]]], 1).reshape(-1, 3)
    return verts.astype(np.int32), tris.astype(np.uint32), np.repeat(Q[:, 1], 2).astype(np.int32)


def grid_voxels(occ, materials=None):
    """A boolean (n, n, n) grid (indexed [x, y, z]) as a Morton-sorted voxel list; materials: an int grid of material + 1."""
    p = np.argwhere(occ)
    m = materials[occ] if materials is not None else np.ones(len(p), np.int64)
    return fm._sorted(np.concatenate([p, np.asarray(m).reshape(-1, 1)], 1).astype(np.int32))
