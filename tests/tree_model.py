"""Test helpers: a numpy restatement of the host's octree builder (csrc/host_scene.cpp build_octree), so that a test can make
trees the scene generators do not (depth 10) without the GPU builder, and the scene payloads around such a tree as
Octree::init_global_buffers writes them (octree.rs:44-100).  tests/test_tree_model.py pins the builder to the host's bytes."""
import numpy as np

from tdt4230_project_raytracing_amd import host

EMPTY, PARENT, LEAF = 0, 1, 2
MIXED = 255                                   # a block that is neither empty nor one material (host_scene.cpp MIXED)

_CHILD = np.array([[c >> 2, (c >> 1) & 1, c & 1] for c in range(8)], np.int64)      # node index in a cell = x * 4 + y * 2 + z


def _key(p, level):
    n = np.int64(1) << level
    return (p[..., 0] * n + p[..., 1]) * n + p[..., 2]


def build_cells(vox, depth):
    """uint32 cells payload {value, type} x 8 nodes per cell of the tree over the (n, 4) voxels {x, y, z, material + 1} on the
    2^depth grid: breadth-first, cell 0 the root cell, a uniformly filled block one LEAF at its own level.  Sparse: only the
    occupied blocks of each level are held, so a depth-10 tree costs what its voxels cost."""
    vox = np.asarray(vox, np.int64).reshape(-1, 4)
    assert depth >= 1 and ((vox[:, :3] >= 0) & (vox[:, :3] < (1 << depth))).all() and ((vox[:, 3] >= 1) & (vox[:, 3] < MIXED)).all()
    # the pyramid: per level the sorted keys of its occupied blocks and their state (material + 1, or MIXED)
    keys, state = [None] * (depth + 1), [None] * (depth + 1)
    k = _key(vox[:, :3], depth)
    order = np.argsort(k, kind="stable")
    k, s, p = k[order], vox[order, 3], vox[order, :3]
    assert (np.diff(k) > 0).all(), "a voxel is listed twice"
    keys[depth], state[depth] = k, s
    for level in range(depth - 1, 0, -1):
        pp = p >> 1
        pk = _key(pp, level)
        order = np.argsort(pk, kind="stable")
        pk, s, pp = pk[order], s[order], pp[order]
        first = np.flatnonzero(np.concatenate([[True], pk[1:] != pk[:-1]])) if pk.size else np.zeros(0, np.int64)
        count = np.diff(np.concatenate([first, [pk.size]]))
        lo, hi = (np.minimum.reduceat(s, first), np.maximum.reduceat(s, first)) if pk.size else (s, s)
        uniform = (count == 8) & (lo == hi) & (lo != MIXED)           # all eight children one material: the block is that material
        k, p = pk[first], pp[first]
        s = np.where(uniform, lo, MIXED)
        keys[level], state[level] = k, s

    out = []
    base = np.zeros((1, 3), np.int64)         # the cells of this level, in breadth-first order: coordinates of their first node
    next_cell = 1
    for level in range(1, depth + 1):
        pos = base[:, None, :] + _CHILD[None, :, :]                   # (m, 8, 3)
        pk = _key(pos, level)
        at = np.searchsorted(keys[level], pk)
        at_c = np.minimum(at, max(len(keys[level]) - 1, 0))
        found = (keys[level][at_c] == pk) if len(keys[level]) else np.zeros(pk.shape, bool)
        st = np.where(found, state[level][at_c] if len(keys[level]) else 0, 0)
        par = st == MIXED
        assert not (par.any() and level == depth)
        nodes = np.zeros(pos.shape[:2] + (2,), np.uint32)
        nodes[..., 1] = np.where(st == 0, EMPTY, np.where(par, PARENT, LEAF))
        nodes[..., 0] = np.where(st == 0, 0, np.where(par, 0, st - 1))
        n_par = int(par.sum())
        nodes[..., 0][par] = next_cell + np.arange(n_par, dtype=np.uint32)      # row-major over (cell, node): the queue's order
        next_cell += n_par
        out.append(nodes.reshape(-1))
        base = pos[par] * 2
        if n_par == 0:
            break
    return np.concatenate(out).astype(np.uint32)


def scene_from_cells(cells, depth, cell_count, like, min_point=(-0.5, -0.5, -1.0), scale=1.0, max_iter=None):
    """host.Scene around `cells`: the material, albedo, metal and dielectric tables of `like`, OctreeFloats = {min_point, 0, scale,
    1 / scale, 1 / cell_count as f32} and OctreeInts = {max_depth, max_iter, cell_count} (octree.rs:44-50, 76-81)."""
    cells = np.ascontiguousarray(cells, np.uint32).reshape(-1)
    assert cells.size % 16 == 0
    blobs = {k: like.blobs[k].copy() for k in (1, 2, 3, 4)}
    blobs[0] = cells
    mp = np.asarray(min_point, np.float32)
    f32 = np.float32
    blobs[6] = np.array([mp[0], mp[1], mp[2], f32(0.0), f32(scale), f32(1.0) / f32(scale), f32(1.0) / f32(cell_count)], np.float32)
    blobs[7] = np.array([depth, like.max_iter if max_iter is None else max_iter, cell_count], np.int32)
    typ = cells.reshape(-1, 2)[:, 1]
    counts = {"cells": cells.size // 16, "parents": int((typ == PARENT).sum()), "leaves": int((typ == LEAF).sum()),
              "empties": int((typ == EMPTY).sum()), "materials": int(blobs[1].size // 3), "voxels": -1}
    return host.Scene(blobs, counts, f"cells_d{depth}_cc{cell_count}")


def with_corner(scene, corner):
    """The same scene with the octree's min corner at `corner` (three float32s, taken bit for bit: -0.0 stays -0.0)."""
    blobs = {k: v.copy() for k, v in scene.blobs.items()}
    blobs[6][:3] = np.asarray(corner, np.float32)
    return host.Scene(blobs, scene.counts, scene.name + "_placed")


def parents_at_level(cells, level):
    """Number of PARENT nodes at tree level `level` (the root cell's nodes are level 1): follows the PARENTs down from cell 0."""
    c = np.asarray(cells, np.uint32).reshape(-1, 8, 2)
    cell = np.zeros(1, np.int64)
    for _ in range(1, level):
        nodes = c[cell]
        cell = nodes[..., 0][nodes[..., 1] == PARENT].astype(np.int64)
        if cell.size == 0:
            return 0
    return int((c[cell][..., 1] == PARENT).sum())
