"""The numpy model of connected components (include/tdt_rt.h tdt_octree_components / tdt_octree_edit_connected), the yardstick
of the GPU tests: neighbours by np.searchsorted on Morton keys, then min-label propagation with pointer jumping.  numpy only."""
import numpy as np

from test_gpu_region_edit import inside, morton, sort_vox
from tdt4230_project_raytracing_amd import rt

MATCH_ANY, MATCH_MATERIAL = 0, 1


def half_offsets(connectivity):
    """The lexicographically positive half of the neighbour offsets: 3 of 6, 13 of 26."""
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) > (0, 0, 0)]
    if connectivity == 6:
        offs = [d for d in offs if sum(map(abs, d)) == 1]
    return np.array(offs, np.int64)


def edges(V, depth, connectivity, match):
    """(a, b) index pairs of connected neighbours in V (Morton-sorted {x, y, z, m}), each unordered pair once."""
    V = np.asarray(V, np.int64).reshape(-1, 4)
    n, N = len(V), 1 << depth
    keys = morton(V[:, :3]).astype(np.int64)
    aa, bb = [], []
    for d in half_offsets(connectivity):
        q = V[:, :3] + d
        idx = np.flatnonzero(((q >= 0) & (q < N)).all(1))
        if not len(idx) or not n:
            continue
        kq = morton(q[idx]).astype(np.int64)
        j = np.minimum(np.searchsorted(keys, kq), n - 1)
        found = keys[j] == kq
        a, b = idx[found], j[found]
        if match == MATCH_MATERIAL:
            same = V[a, 3] == V[b, 3]
            a, b = a[same], b[same]
        aa.append(a)
        bb.append(b)
    if not aa:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(aa), np.concatenate(bb)


def root_of(n, a, b):
    """The lowest index of each voxel's component: stars hooked onto their lowest neighbouring root, then pointer jumping."""
    parent = np.arange(n, dtype=np.int64)
    while len(a):
        pa, pb = parent[a], parent[b]
        lo, hi = np.minimum(pa, pb), np.maximum(pa, pb)
        live = lo != hi
        a, b, lo, hi = a[live], b[live], lo[live], hi[live]
        if not len(a):
            break
        np.minimum.at(parent, hi, lo)                         # hi is a root (every tree is a star here), lo < hi
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent


def components(V, depth, connectivity=6, match=MATCH_ANY):
    """(labels uint32, table of rt.COMPONENT_DTYPE) as tdt_octree_components defines them."""
    V = np.asarray(V, np.int64).reshape(-1, 4)
    n = len(V)
    a, b = edges(V, depth, connectivity, match)
    root = root_of(n, a, b)
    roots = np.flatnonzero(root == np.arange(n))
    labels = np.searchsorted(roots, root)
    tab = np.zeros(len(roots), rt.COMPONENT_DTYPE)
    tab["first"] = roots
    tab["material"] = V[roots, 3] if n else []
    tab["voxels"] = np.bincount(labels, minlength=len(roots))
    if n:
        order = np.argsort(labels, kind="stable")
        starts = np.searchsorted(labels[order], np.arange(len(roots)))
        for ax in range(3):
            c = V[order, ax]
            tab["lo"][:, ax] = np.minimum.reduceat(c, starts)
            tab["hi"][:, ax] = np.maximum.reduceat(c, starts)
    return labels.astype(np.uint32), tab


def selected(V, depth, labels, tab, seeds=None, regions=None, min_voxels=0, max_voxels=2**32 - 1, invert=False):
    """The selection rule over the components: a bool per component."""
    V = np.asarray(V, np.int64).reshape(-1, 4)
    size = tab["voxels"].astype(np.int64)
    sel = (size >= min_voxels) & (size <= max_voxels)
    if seeds is not None and len(np.asarray(seeds).reshape(-1, 3)):
        s = np.asarray(seeds, np.int64).reshape(-1, 3)
        N = 1 << depth
        s = s[((s >= 0) & (s < N)).all(1)]
        keys = morton(V[:, :3]).astype(np.int64)
        hit = np.zeros(len(tab), bool)
        if len(s) and len(V):
            ks = morton(s).astype(np.int64)
            j = np.minimum(np.searchsorted(keys, ks), len(V) - 1)
            hit[labels[j[keys[j] == ks]]] = True
        sel &= hit
    if regions is not None and len(regions):
        touch = np.zeros(len(tab), bool)
        touch[labels[inside(V[:, :3], regions)]] = True
        sel &= touch
    return sel != bool(invert)


def edit(V, depth, op, material=0, connectivity=6, match=MATCH_ANY, **select):
    """The voxel list tdt_octree_edit_connected leaves (op REGION_PAINT / REGION_CLEAR), Morton-sorted."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    labels, tab = components(V, depth, connectivity, match)
    member = selected(V, depth, labels, tab, **select)[labels] if len(V) else np.zeros(0, bool)
    if op == rt.REGION_CLEAR:
        return sort_vox(V[~member])
    out = V.copy()
    out[member, 3] = material + 1
    return sort_vox(out)


def extract(V, depth, connectivity=6, match=MATCH_ANY, **select):
    """What tdt_octree_extract_connected returns."""
    V = np.asarray(V, np.int32).reshape(-1, 4)
    labels, tab = components(V, depth, connectivity, match)
    member = selected(V, depth, labels, tab, **select)[labels] if len(V) else np.zeros(0, bool)
    return np.ascontiguousarray(V[member])

