"""Geodesic distance (include/tdt_rt.h tdt_octree_geodesic_field / tdt_octree_extract_geodesic / tdt_octree_edit_geodesic /
tdt_octree_geodesic_path) without a GPU: the ABI, the numpy model (tests/geodesic_model.py) against a plain heapq Dijkstra,
against closed forms in free space and against the models of its two neighbours (connected components, enclosed space), the
canonical path's own properties, the kernels' resources, and the unit compiled for the CPU under the sanitizers."""
import ctypes
import heapq
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import connect_model as cm
import fill_model as fm
import geodesic_model as gm
from test_gpu_region_edit import sort_vox
from tdt4230_project_raytracing_amd import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_octree_geodesic_field", "tdt_octree_extract_geodesic", "tdt_octree_edit_geodesic", "tdt_octree_geodesic_path",
         "tdt_debug_geodesic_passes")
WEIGHTS = ((1, 0, 0), (1, 1, 1), (3, 4, 5), (2, 3, 0), (5, 1, 1), (7, 0, 2))
BIG = 1 << 30


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_geodesic_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    for n in ("octree_geodesic_field", "octree_extract_geodesic", "octree_edit_geodesic", "octree_geodesic_path", "geodesic_passes"):
        assert callable(getattr(rt.Context, n)), n
    assert (rt.MEDIUM_EMPTY, rt.MEDIUM_SOLID) == (0, 1) and rt.GEODESIC_DOMAIN_CAP == 1 << 27
    assert (rt.STEPS_6, rt.STEPS_26, rt.CHAMFER_345) == ((1, 0, 0), (1, 1, 1), (3, 4, 5))


def test_geodesic_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_geodesic \{(.*?)\} tdt_geodesic;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"int32_t\s+([^;]+);", body):
        for name, count in re.findall(r"(\w+)(?:\[(\d+)\])?", decl):
            fields.append((name, int(count or 1)))
    assert fields == [("medium", 1), ("match", 1), ("w", 3), ("max_cost", 1), ("material", 1), ("pad", 1)]
    assert [(n, ctypes.sizeof(t) // 4) for n, t in rt.Geodesic._fields_] == fields
    assert ctypes.sizeof(rt.Geodesic) == 32 and "static_assert(sizeof(tdt_geodesic) == 32" in text
    assert re.search(r"#define TDT_GEODESIC_DOMAIN_CAP \(1u << 27\)", text)
    assert re.search(r"enum \{ TDT_MEDIUM_EMPTY = 0, TDT_MEDIUM_SOLID = 1 \};", text)


def test_python_wrapper_argument_checks():
    g, s, k = rt.Context._geodesic(rt.MEDIUM_EMPTY, rt.CHAMFER_345, 48, None, 7, [(1, 2, 3), (4, 5, 6)])
    assert (g.medium, g.match, list(g.w), g.max_cost, g.material, g.pad) == (0, -1, [3, 4, 5], 48, 7, 0)
    assert k == 2 and s.dtype == np.int32 and s.tolist() == [[1, 2, 3], [4, 5, 6]]
    g, s, k = rt.Context._geodesic(rt.MEDIUM_SOLID, (1, 0, 0), 0, 5, None, [])
    assert (g.match, g.material, k) == (5, -1, 0)
    for bad in (dict(steps=(1, 2)), dict(steps=(1, 2.5, 0)), dict(max_cost=2 ** 31), dict(medium=True), dict(seeds=[(1.5, 0, 0)]),
                dict(seeds=[(2 ** 31, 0, 0)])):
        kw = dict(medium=1, steps=(1, 0, 0), max_cost=1, match=None, material=None, seeds=[(0, 0, 0)])
        kw.update(bad)
        with pytest.raises(ValueError):
            rt.Context._geodesic(**kw)


# ---- the model against a plain Dijkstra ----------------------------------------------------------------------------------------
def dijkstra(P, seeds, w, max_cost):
    """g by the textbook algorithm on python tuples: the model's yardstick."""
    n = P.shape[0]
    g = {}
    heap = []
    for s in seeds:
        s = tuple(int(v) for v in s)
        if all(0 <= v < n for v in s) and P[s]:
            g[s] = 0
            heap.append((0, s))
    heapq.heapify(heap)
    while heap:
        c, p = heapq.heappop(heap)
        if c != g[p]:
            continue
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    k = abs(dx) + abs(dy) + abs(dz) - 1
                    if k < 0 or not w[k]:
                        continue
                    q = (p[0] + dx, p[1] + dy, p[2] + dz)
                    if all(0 <= v < n for v in q) and P[q] and c + w[k] < g.get(q, 1 << 60):
                        g[q] = c + w[k]
                        heapq.heappush(heap, (c + w[k], q))
    out = np.full(P.shape, -1, np.int64)
    for q, c in g.items():
        if c <= max_cost:
            out[q] = c
    return out


def random_list(depth, seed, density=0.6):
    rng = np.random.default_rng(seed)
    n = 1 << depth
    p = np.argwhere(rng.random((n, n, n)) < density)
    return sort_vox(np.concatenate([p, 1 + rng.integers(0, 3, (len(p), 1))], 1))


@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("n", [8, 12])
def test_model_equals_a_plain_dijkstra(n, w):
    rng = np.random.default_rng(100 * n + sum(w))
    mat = np.where(rng.random((n, n, n)) < 0.6, 1 + rng.integers(0, 3, (n, n, n)), 0)
    p = np.argwhere(mat > 0)
    V = sort_vox(np.concatenate([p, mat[p[:, 0], p[:, 1], p[:, 2]][:, None]], 1))
    mask = [rt.box((1, 0, 2), (n - 3, n - 2, n - 1)), rt.sphere((n // 2, n // 2, n // 3), n // 3)]
    from test_gpu_region_edit import inside
    cells = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    in_mask = inside(cells, mask).reshape(n, n, n)
    differed = 0
    for medium, match, masked, max_cost in ((gm.SOLID, None, False, BIG), (gm.EMPTY, None, False, BIG), (gm.SOLID, 1, False, BIG),
                                            (gm.EMPTY, None, True, BIG), (gm.SOLID, None, True, 9), (gm.EMPTY, None, False, 7),
                                            (gm.SOLID, None, False, 0)):
        seeds = np.concatenate([rng.integers(0, n, (5, 3)), [[-1, 0, 0], [0, n, 0]]])
        P = mat == 0 if medium == gm.EMPTY else (mat > 0 if match is None else mat == match + 1)
        P = P & in_mask if masked else P
        if n == 8:                                               # a whole grid of depth 3: the model's own medium and forms
            Pm, g = gm.solve(V, 3, seeds, medium, w, max_cost, match, mask if masked else None)
            assert np.array_equal(Pm, P)
            lo, hi = (1, 0, 2), (6, 7, 5)
            f = gm.field(V, 3, seeds, lo, hi, g=g)
            assert f.shape == (4, 8, 6) and np.array_equal(f, g[1:7, 0:8, 2:6].transpose(2, 1, 0))
            if medium == gm.SOLID:
                own = gm.reach_list(V, 3, seeds, g=g)
                assert np.array_equal(own, V[g[V[:, 0], V[:, 1], V[:, 2]] >= 0])
                assert np.array_equal(gm.reach_list(V, 3, seeds, material=9, g=g), np.concatenate([own[:, :3], np.full((len(own), 1), 10)], 1))
        else:
            g = gm.distances(P, seeds, w, max_cost)
        want = dijkstra(P, seeds, w, max_cost)
        assert np.array_equal(g, want), (medium, match, max_cost)
        assert ((g >= 0) <= P).all() and (g <= max_cost).all()
        differed += int((g > 0).any())
    assert differed >= 4                                         # the cases are not vacuous
    if n == 8:
        assert not gm.medium_of(V, 3, gm.SOLID, None, []).any()  # an empty mask


# ---- closed forms in free space ------------------------------------------------------------------------------------------------
def test_closed_forms_in_free_space():
    n, depth = 13, 4
    seed = np.array([5, 7, 6])
    P = np.zeros((16, 16, 16), bool)
    P[:n, :n, :n] = True
    d = np.sort(np.abs(np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1) - seed), -1)
    c, b, a = d[..., 0], d[..., 1], d[..., 2]                    # a >= b >= c
    for w, want in (((1, 0, 0), a + b + c), ((1, 1, 1), a), ((3, 4, 5), 3 * a + b + c)):
        g = gm.distances(P, [seed], w)
        assert np.array_equal(g[:n, :n, :n], want[:n, :n, :n]), w
        assert np.array_equal(g, dijkstra(P, [seed], w, BIG)), w
        assert (g[n:] == -1).all() and (g[:, n:] == -1).all() and (g[:, :, n:] == -1).all()


# ---- the two neighbours --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity,w", [(6, (1, 0, 0)), (26, (1, 1, 1))])
def test_solid_reach_is_the_connected_component_of_the_seeds(connectivity, w):
    depth = 4
    V = random_list(depth, 5, 0.22 if connectivity == 6 else 0.06)
    seeds = V[[3, len(V) // 2, len(V) - 7], :3]
    got = gm.reach_list(V, depth, seeds, steps=w)
    want = cm.extract(V, depth, connectivity, seeds=seeds)
    assert np.array_equal(got, sort_vox(want)) and 3 <= len(got) < len(V)
    per_material = gm.reach_list(V, depth, seeds[:1], steps=w, match=int(V[3, 3]) - 1)
    assert np.array_equal(per_material, sort_vox(cm.extract(V, depth, connectivity, cm.MATCH_MATERIAL, seeds=seeds[:1])))


@pytest.mark.parametrize("connectivity,w", [(6, (1, 0, 0)), (26, (1, 1, 1))])
def test_empty_reach_from_the_faces_is_the_complement_of_the_enclosed_set(connectivity, w):
    depth, n = 4, 16
    V = random_list(depth, 9, 0.6 if connectivity == 6 else 0.9)
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    faces = g[((g == 0) | (g == n - 1)).any(1)]
    reach = gm.solve(V, depth, faces, gm.EMPTY, w)[1] >= 0
    empty = gm.grid_of(V, depth) == 0
    E = fm.enclosed_grid(V, depth, connectivity)
    assert np.array_equal(reach, empty & ~E) and E.any() and reach.any()


# ---- the canonical path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WEIGHTS)
def test_canonical_path_is_a_valid_step_sequence(w):
    depth = 4
    V = random_list(depth, 31, 0.7)
    seeds = V[[1, len(V) // 3], :3]
    P, g = gm.solve(V, depth, seeds, steps=w)
    far = np.argwhere(g == g.max())[0]
    assert g.max() > 3 * min(v for v in w if v)
    pts, cost = gm.path(V, depth, seeds, far, steps=w, g=g)
    assert cost == g[tuple(far)] and tuple(pts[0]) == tuple(far) and g[tuple(pts[-1])] == 0
    assert any(tuple(pts[-1]) == tuple(s) for s in seeds)
    total = 0
    for p, q in zip(pts[:-1], pts[1:]):
        d = np.abs(q.astype(int) - p.astype(int))
        assert d.max() == 1 and P[tuple(p)] and P[tuple(q)] and w[d.sum() - 1] > 0
        total += w[d.sum() - 1]
    assert total == cost
    assert gm.path(V, depth, seeds, (-1, 0, 0), steps=w, g=g)[1] == -1
    unreached = np.argwhere(g < 0)[0]
    none, c = gm.path(V, depth, seeds, unreached, steps=w, g=g)
    assert len(none) == 0 and c == -1
    one, c = gm.path(V, depth, seeds, seeds[0], steps=w, g=g)
    assert one.tolist() == [seeds[0].tolist()] and c == 0


def test_domain_box_rule():
    depth = 5
    V = sort_vox(np.array([[4, 5, 6, 1], [20, 9, 30, 2]], np.int32))
    seeds = [(10, 8, 8), (12, 40, 8)]                            # the second is off the grid
    assert gm.domain_box(V, depth, seeds, gm.EMPTY, (3, 4, 5), 10) == ((7, 5, 5), (13, 11, 11))
    assert gm.domain_box(V, depth, seeds, gm.EMPTY, (5, 1, 2), 3) == ((7, 5, 5), (13, 11, 11))
    assert gm.domain_box(V, depth, seeds, gm.SOLID, (1, 0, 0), 3) == ((7, 5, 6), (13, 9, 11))
    assert gm.domain_box(V, depth, seeds, gm.EMPTY, (1, 0, 0), BIG) == ((0, 0, 0), (31, 31, 31))
    assert gm.domain_box(V, depth, seeds, gm.EMPTY, (1, 0, 0), BIG, regions=[rt.box((9, -4, 0), (50, 8, 8)), rt.sphere((9, 9, 9), 1)]) == ((8, 0, 0), (31, 10, 10))
    assert gm.domain_box(V, depth, seeds, gm.EMPTY, (1, 0, 0), BIG, regions=[]) is None
    assert gm.domain_box(V, depth, [(40, 0, 0)], gm.EMPTY, (1, 0, 0), BIG) is None
    assert gm.domain_box(V[:0], depth, seeds, gm.SOLID, (1, 0, 0), BIG) is None
    assert gm.domain_box(V, depth, [(0, 0, 0)], gm.SOLID, (1, 0, 0), 2) is None


# ---- the kernels and the unit --------------------------------------------------------------------------------------------------
def test_geodesic_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_geodesic.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {n for n in names if n.startswith("geo_")} == {"geo_medium_kernel", "geo_init_kernel", "geo_seed_kernel", "geo_relax_kernel",
                                                          "geo_reach_kernel", "geo_count_kernel", "geo_emit_kernel", "geo_field_kernel",
                                                          "geo_path_kernel"}
    assert not {n for n in names if n.startswith("bitvol_")}     # the shared steps: test_bitvol_api.py has the bit volume's kernels to itself
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


def test_the_unit_compiled_for_the_cpu_runs_clean_under_the_sanitizers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostsim", "run.py"), "geodesic"], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout and "MISMATCH" not in r.stdout and "ERROR" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
