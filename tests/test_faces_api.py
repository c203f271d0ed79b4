"""Face tools without a GPU: the entry points are exported and bound, the Python struct layouts and constants are the header's, the
unit is part of the device library and its kernels cross-compile without scratch or spills, the wrapper refuses every bad argument
the header lists, the numpy model the GPU tests compare against (tests/faces_model.py) equals an independent dense brute force and
the closed forms of the definition, and tdt_pick_face turns hand-made hits into seeds."""
import ctypes
import os
import re
import sys
from collections import deque

import numpy as np
import pytest

import faces_model as fm
import surface_model as sm
from test_gpu_region_edit import morton, sort_vox
from tdt4230_project_raytracing_amd import build, host, rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_octree_face_regions", "tdt_octree_extract_faces", "tdt_octree_edit_faces", "tdt_debug_faces_premerge")
KINDS = [(c, m) for c in (4, 8) for m in (rt.MATCH_ANY, rt.MATCH_MATERIAL)]


@pytest.fixture(autouse=True)
def model_states_the_library_contract():
    assert (fm.MATCH_ANY, fm.MATCH_MATERIAL) == (rt.MATCH_ANY, rt.MATCH_MATERIAL)
    assert (fm.COLUMNS, fm.TREE, fm.DISTANCE_MAX) == (rt.FACES_COLUMNS, rt.FACES_TREE, rt.FACES_DISTANCE_MAX)


def block(lo, hi, m=1):
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([g, np.full((len(g), 1), m)], 1).astype(np.int32)


# ---- 1. exports, layouts, kernels ---------------------------------------------------------------------------------------------
def test_faces_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    assert "tdt_faces.hip" in build.DEVICE_UNITS
    assert os.path.exists(os.path.join(build.CSRC, "tdt_faces.hip"))
    assert {"surface_device.hpp", "unionfind_device.hpp"} <= set(build.DEVICE_HEADERS)
    assert hasattr(host.lib(), "tdt_pick_face")
    assert re.search(r"\bint tdt_pick_face\s*\(", open(os.path.join(ROOT, "include", "tdt_host.h")).read())


def header_fields(text, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for kind, names in re.findall(r"(u?int32_t)\s+([^;]+);", body):
        for f in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", f)
            fields.append((kind, m.group(1), int(m.group(2) or 1)))
    return fields


def test_faces_structs_and_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    for name, cls, size, dtype in (("tdt_faces", rt.Faces, 24, None), ("tdt_face_region", rt.FaceRegion, 40, rt.FACE_REGION_DTYPE)):
        fields = header_fields(text, name)
        assert [f[1] for f in fields] == [f[0] for f in cls._fields_]
        offset = 0
        for kind, field, count in fields:
            base = ctypes.c_uint32 if kind == "uint32_t" else ctypes.c_int32
            assert getattr(cls, field).offset == offset, field
            assert dict(cls._fields_)[field] is (base if count == 1 else base * count), field
            if dtype is not None:
                assert dtype.fields[field][1] == offset and dtype.fields[field][0].base == np.dtype("<u4" if kind == "uint32_t" else "<i4")
            offset += 4 * count
        assert offset == ctypes.sizeof(cls) == size
        assert len(re.findall(rf"sizeof\({name}\) == {size}", text)) == 2          # C++ and C
    assert [f[1] for f in header_fields(text, "tdt_faces")] == ["connectivity", "match", "distance", "block", "material", "pad"]
    assert re.search(r"#define TDT_FACES_DISTANCE_MAX 1023\b", text) and rt.FACES_DISTANCE_MAX == 1023
    assert re.search(r"enum \{ TDT_FACES_COLUMNS = 0, TDT_FACES_TREE = 1 \};", text) and (rt.FACES_COLUMNS, rt.FACES_TREE) == (0, 1)


def test_faces_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_faces.hip")
    names = {re.match(r"(?:void )?tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"faces_init_kernel", "faces_hook_kernel", "faces_table_init_kernel", "faces_table_kernel", "faces_seed_kernel", "faces_count_kernel",
            "faces_emit_kernel", "faces_list_kernel"} <= names
    assert sum("faces_hook_kernel<" in r["name"] for r in rows) == 4          # connectivity 4 / 8 x with / without the pre-merge
    assert sum("faces_init_kernel<" in r["name"] for r in rows) == 2
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]
    # the probe, the emit and the union-find are shared, not copied: the unit's source defines none of them
    src = open(os.path.join(build.CSRC, "tdt_faces.hip")).read()
    for shared in ("surface_probe_kernel", "surface_emit_kernel", "uint32_t uf_find", "void uf_unite", "struct SurfaceSegs"):
        assert shared not in src, shared
    assert not any("surface_probe_kernel" in r["name"] or "surface_emit_kernel" in r["name"] for r in rows)


# ---- 2. the wrapper's argument checks -----------------------------------------------------------------------------------------
def test_python_wrapper_argument_checks():
    seeds = np.array([[1, 2, 3, 0], [4, 5, 6, 5]], np.int32)
    f, s = rt._faces(seeds, -7, 8, rt.MATCH_ANY, True, 253, what=rt.FACES_TREE, op=rt.REGION_CLEAR)
    assert (f.connectivity, f.match, f.distance, f.block, f.material, f.pad) == (8, rt.MATCH_ANY, -7, 1, 253, 0)
    assert s.dtype == np.int32 and s.flags["C_CONTIGUOUS"] and np.array_equal(s, seeds)
    f, s = rt._faces([1, 2, 3, 4], rt.FACES_DISTANCE_MAX)                    # one seed as a flat quadruple
    assert (f.connectivity, f.match, f.block, f.material) == (4, rt.MATCH_MATERIAL, 0, -1) and s.shape == (1, 4)
    f, s = rt._faces(np.zeros((0, 4), np.int32), -rt.FACES_DISTANCE_MAX)
    assert s.shape == (0, 4) and f.distance == -1023
    for bad in (lambda: rt._faces(seeds.astype(np.float32), 1),
                lambda: rt._faces(seeds[:, :3], 1),
                lambda: rt._faces(seeds.astype(np.int64) + 2 ** 40, 1),
                lambda: rt._faces([[1, 2, 3, 6]], 1), lambda: rt._faces([[1, 2, 3, -1]], 1),           # a seed f outside 0..5
                lambda: rt._faces(np.zeros(((1 << 20) + 1, 4), np.int32), 1),                          # more than 2^20 seeds
                lambda: rt._faces(seeds, 1, 6), lambda: rt._faces(seeds, 1, 26), lambda: rt._faces(seeds, 1, 0), lambda: rt._faces(seeds, 1, 4.5),
                lambda: rt._faces(seeds, 1, 4, 2), lambda: rt._faces(seeds, 1, 4, -1),
                lambda: rt._faces(seeds, rt.FACES_DISTANCE_MAX + 1), lambda: rt._faces(seeds, -rt.FACES_DISTANCE_MAX - 1),
                lambda: rt._faces(seeds, 1.5), lambda: rt._faces(seeds, True), lambda: rt._faces(seeds, 2 ** 31),
                lambda: rt._faces(seeds, 1, block=2), lambda: rt._faces(seeds, 1, block=-1),
                lambda: rt._faces(seeds, 1, material=-2), lambda: rt._faces(seeds, 1, material=254), lambda: rt._faces(seeds, 1, material=None),
                lambda: rt._faces(seeds, 1, what=2), lambda: rt._faces(seeds, 1, what=-1),
                lambda: rt._faces(seeds, 1, op=4), lambda: rt._faces(seeds, 1, op=-1)):
        with pytest.raises(ValueError):
            bad()


# ---- 3. the model against a dense brute force ---------------------------------------------------------------------------------
def brute_regions(occ, mat, connectivity, match):
    """Per direction and per w a 2-D breadth-first search over a dense plane.  Returns the face records in F's order as tuples
    (f, w, u, v, m, (x, y, z)), their labels, and per region [first, faces, f, w, lo_u, lo_v, hi_u, hi_v, m]."""
    n = occ.shape[0]
    recs, labels, table = [], [], []
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    for f in range(6):
        a, s, ua, va = f >> 1, f & 1, ((f >> 1) + 1) % 3, ((f >> 1) + 2) % 3
        for w in range(n):
            plane = np.zeros((n, n), bool)
            pm = np.zeros((n, n), int)
            for u in range(n):
                for v in range(n):
                    p = [0, 0, 0]
                    p[a], p[ua], p[va] = w, u, v
                    if not occ[tuple(p)]:
                        continue
                    q = list(p)
                    q[a] += 1 if s else -1
                    if 0 <= q[a] < n and occ[tuple(q)]:
                        continue
                    plane[u, v] = True
                    pm[u, v] = mat[tuple(p)]
            lab = -np.ones((n, n), int)
            base = len(recs)
            order = [(u, v) for u in range(n) for v in range(n) if plane[u, v]]
            index = {uv: base + i for i, uv in enumerate(order)}
            for (u, v) in order:                                   # in F's order: a new search starts at each region's first face
                if lab[u, v] >= 0:
                    continue
                r = len(table)
                table.append([index[(u, v)], 0, f, w, u, v, u, v, pm[u, v]])
                lab[u, v] = r
                todo = deque([(u, v)])
                while todo:
                    cu, cv = todo.popleft()
                    t = table[r]
                    t[1] += 1
                    t[4], t[5], t[6], t[7] = min(t[4], cu), min(t[5], cv), max(t[6], cu), max(t[7], cv)
                    for du, dv in steps:
                        nu, nv = cu + du, cv + dv
                        if 0 <= nu < n and 0 <= nv < n and plane[nu, nv] and lab[nu, nv] < 0 and \
                                (match == rt.MATCH_ANY or pm[nu, nv] == pm[cu, cv]):
                            lab[nu, nv] = r
                            todo.append((nu, nv))
            for (u, v) in order:
                p = [0, 0, 0]
                p[a], p[ua], p[va] = w, u, v
                recs.append((f, w, u, v, pm[u, v], tuple(p)))
                labels.append(lab[u, v])
    return recs, labels, table


def brute_columns(occ, recs, labels, chosen, distance, block, material):
    """Explicit loops: every selected face in F's order, k ascending, a dict taking the last value per voxel."""
    n = occ.shape[0]
    out = {}
    for (f, w, u, v, m, p), lab in zip(recs, labels):
        if lab not in chosen:
            continue
        step = (1 if f & 1 else -1) * (1 if distance > 0 else -1)
        for k in range(abs(distance)):
            q = list(p)
            q[f >> 1] += step * (k + 1 if distance > 0 else k)
            if not 0 <= q[f >> 1] < n:
                break
            if block and bool(occ[tuple(q)]) == (distance > 0):
                break
            out[tuple(q)] = m if material < 0 else material + 1
    rows = np.array([[*p, m] for p, m in out.items()], np.int32).reshape(-1, 4)
    return sort_vox(rows)


@pytest.mark.parametrize("n,fill", [(8, 0.3), (8, 0.6), (8, 0.9), (16, 0.3), (16, 0.6), (16, 0.9)])
def test_model_equals_a_dense_brute_force(n, fill):
    rng = np.random.default_rng(int(n * 100 + fill * 10))
    depth = n.bit_length() - 1
    occ = rng.random((n, n, n)) < fill
    mat = rng.integers(1, 4, (n, n, n))
    V = sm.grid_voxels(occ, mat)
    F = fm.face_list(V, depth)
    for conn, match in KINDS:
        recs, labels, table = brute_regions(occ, mat, conn, match)
        got_l, got_t = fm.face_regions(F, depth, conn, match)
        assert [r[:5] for r in recs] == [tuple(int(c) for c in row[:5]) for row in F]
        assert [tuple(int(c) for c in V[row[5], :3]) for row in F] == [r[5] for r in recs]
        assert got_l.tolist() == labels
        want_t = np.array(table, np.int64).reshape(-1, 9)
        assert np.array_equal(np.stack([got_t["first"], got_t["faces"], got_t["face"], got_t["w"], got_t["lo"][:, 0], got_t["lo"][:, 1],
                                        got_t["hi"][:, 0], got_t["hi"][:, 1], got_t["material"]], 1).astype(np.int64), want_t)
        # the guard: more than one region per direction, and some region of more than one face
        for f in range(6):
            assert (got_t["face"] == f).sum() > 1
        assert got_t["faces"].max() > 1
        # seeds: three faces of different regions, a duplicate, an empty voxel, a buried or absent face, a voxel off the grid
        pick = rng.choice(len(F), 3, replace=False)
        seeds = [[*V[F[i, 5], :3], F[i, 0]] for i in pick] + [[*V[F[pick[0], 5], :3], F[pick[0], 0]]]
        empty = np.argwhere(~occ)
        seeds += [[*empty[0], 1], [n, 0, 0, 0], [-1, 2, 2, 3]]
        chosen = {labels[i] for i in pick}
        sel = fm.selected(F, got_l, len(got_t), seeds)
        assert set(np.flatnonzero(sel)) == chosen
        for distance, blocked, material in ((1, 0, -1), (3, 1, 7), (-2, 1, -1), (-n, 0, 0), (n + 3, 0, -1), (-3, 1, 5)):
            want = brute_columns(occ, recs, labels, chosen, distance, blocked, material)
            got = fm.column_list(V, depth, seeds, distance, conn, match, blocked, material)
            assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (conn, match, distance, blocked, material)


# ---- 4. closed forms -----------------------------------------------------------------------------------------------------------
def test_cube_closed_forms():
    depth, s = 3, 3
    V = sort_vox(block((2, 2, 2), (4, 4, 4), 6))
    F = fm.face_list(V, depth)
    assert np.array_equal(fm.quads(F), sm.quads(V, depth, merge=False))          # F is the surface's face list, row for row
    for conn, match in KINDS:
        labels, tab = fm.face_regions(F, depth, conn, match)
        assert len(tab) == 6 and (tab["faces"] == s * s).all()
        assert tab["first"].tolist() == [0, 9, 18, 27, 36, 45] and tab["face"].tolist() == [0, 1, 2, 3, 4, 5]
        assert tab["w"].tolist() == [2, 4, 2, 4, 2, 4] and (tab["material"] == 6).all()
        assert (tab["lo"] == 2).all() and (tab["hi"] == 4).all()
        assert labels.tolist() == [i // 9 for i in range(54)]
    # pulling +x by d: s^2 d voxels, clipped at the grid face (x = 5, 6, 7 are left)
    for d, depth_x in ((1, 1), (2, 2), (3, 3), (4, 3), (1023, 3)):
        B = fm.column_list(V, depth, [[4, 3, 3, 1]], d)
        assert len(B) == s * s * depth_x and B[:, 0].min() == 5 and B[:, 0].max() == 4 + depth_x and (B[:, 3] == 6).all()
        assert ((B[:, 1:3] >= 2) & (B[:, 1:3] <= 4)).all()
    assert len(fm.edit(V, depth, rt.REGION_FILL, [[4, 3, 3, 1]], 2)) == 27 + 18
    # pushing by -d, d >= s, block = 1 removes exactly the cube, from any side; block = 0 reaches the grid's face
    for seed in ([4, 3, 3, 1], [2, 2, 4, 0], [3, 3, 2, 4], [3, 4, 3, 3]):
        for d in (3, 4, 1023):
            assert np.array_equal(fm.column_list(V, depth, [seed], -d, block=True), V)
            assert len(fm.edit(V, depth, rt.REGION_CLEAR, [seed], -d, block=True)) == 0
            assert np.array_equal(fm.extract(V, depth, [seed], -d, fm.TREE, block=True), V)
    assert len(fm.column_list(V, depth, [[4, 3, 3, 1]], -1023)) == 9 * 5          # x = 4 .. 0
    # d = 0, no seeds, a seed on the cube's inside, on air: nothing
    assert fm.column_list(V, depth, [[4, 3, 3, 1]], 0).shape == (0, 4)
    assert fm.column_list(V, depth, np.zeros((0, 4)), 3).shape == (0, 4)
    assert fm.column_list(V, depth, [[3, 3, 3, 1], [3, 3, 4, 0], [6, 6, 6, 2]], 3).shape == (0, 4)
    # paint a face: d = -1 is the owners
    B = fm.column_list(V, depth, [[3, 3, 4, 5]], -1, material=9)
    assert len(B) == 9 and (B[:, 2] == 4).all() and (B[:, 3] == 10).all()


def test_corner_contact_and_coplanar_opposites():
    depth = 3
    # two 2 x 2 squares in the plane z = 3 touching at a corner
    V = sort_vox(np.concatenate([block((1, 1, 3), (2, 2, 3), 1), block((3, 3, 3), (4, 4, 3), 1)]))
    F = fm.face_list(V, depth)
    for f in (4, 5):
        for conn, want in ((4, 2), (8, 1)):
            _, tab = fm.face_regions(F, depth, conn, rt.MATCH_ANY)
            assert (tab["face"] == f).sum() == want
    assert len(fm.column_list(V, depth, [[1, 1, 3, 5]], 1, 4)) == 4 and len(fm.column_list(V, depth, [[1, 1, 3, 5]], 1, 8)) == 8
    # materials split what connectivity joins
    V2 = V.copy()
    V2[V2[:, 0] >= 3, 3] = 2
    _, tab = fm.face_regions(fm.face_list(V2, depth), depth, 8, rt.MATCH_MATERIAL)
    assert (tab["face"] == 5).sum() == 2
    # a -x face at w = 4 and a +x face at w - 1 = 3 lie in the plane x = 4 and touch along an edge: never one region
    V = sort_vox(np.concatenate([block((4, 2, 2), (4, 3, 3), 1), block((3, 4, 2), (3, 5, 3), 1)]))
    F = fm.face_list(V, depth)
    labels, tab = fm.face_regions(F, depth, 8, rt.MATCH_ANY)
    minus = tab[(tab["face"] == 0) & (tab["w"] == 4)]
    plus = tab[(tab["face"] == 1) & (tab["w"] == 3)]
    assert len(minus) == 1 and len(plus) == 1 and minus["faces"][0] == 4 and plus["faces"][0] == 4
    assert fm.column_list(V, depth, [[4, 2, 2, 0]], 1)[:, 1].max() == 3           # the pull of one does not take the other along


@pytest.mark.parametrize("gap", [3, 4])
def test_slot_walls_pulled_towards_each_other(gap):
    """Two walls facing each other across a slot of `gap` voxels, pulled by the whole gap with their own colours: every slot voxel
    is in a column of each, and the later direction in F (-x, face 0, comes before +x, face 1) wins — so the +x pull of the left
    wall paints all of it."""
    depth = 4
    left, right = block((2, 4, 4), (3, 7, 7), 3), block((4 + gap, 4, 4), (5 + gap, 7, 7), 8)
    V = sort_vox(np.concatenate([left, right]))
    seeds = [[4 + gap, 5, 5, 0], [3, 5, 5, 1]]                     # the right wall's -x face, the left wall's +x face
    B = fm.column_list(V, depth, seeds, gap)
    slot = B[(B[:, 0] >= 4) & (B[:, 0] < 4 + gap)]
    assert len(slot) == len(B) == 16 * gap and (slot[:, 3] == 3).all()
    # each alone keeps its own colour; block = 1 changes nothing (the gap is reached exactly), and a longer blocked pull stops there
    assert (fm.column_list(V, depth, seeds[:1], gap)[:, 3] == 8).all()
    assert np.array_equal(fm.column_list(V, depth, seeds, gap, block=True), B)
    assert np.array_equal(fm.column_list(V, depth, seeds, gap + 5, block=True), B)
    half = fm.column_list(V, depth, seeds, (gap + 1) // 2)         # odd gap: the middle layer is reached by both
    mid = half[half[:, 0] == 4 + gap // 2]
    if gap % 2:
        assert len(mid) == 16 and (mid[:, 3] == 3).all()
    else:
        assert (half[half[:, 0] < 4 + gap // 2, 3] == 3).all() and (half[half[:, 0] >= 4 + gap // 2, 3] == 8).all()
    # the seeds' order does not matter: the order is F's
    assert np.array_equal(fm.column_list(V, depth, seeds[::-1], gap), B)
    key = morton(B[:, :3])
    assert (key[1:] > key[:-1]).all()


# ---- 5. pick_face ----------------------------------------------------------------------------------------------------------------
def _hit(point, normal, status=None, fresh=1):
    rec = np.zeros(1, rt.RAY_HIT_DTYPE)
    rec["status"] = rt.RAY_HIT if status is None else status
    rec["fresh_record"] = fresh
    rec["point"] = point
    rec["normal"] = normal
    return rec[0]


def test_pick_face():
    depth, cells = 4, 16
    floats = np.array([0, 0, 0, 0, 1, 1, 1 / 1024], np.float32)
    ints = np.array([depth, 64, 1024], np.int32)
    k = np.array([5, 9, 12])
    for f in range(6):
        a, s = f >> 1, f & 1
        normal = np.zeros(3, np.float32)
        normal[a] = 1.0 if s else -1.0
        u = (k + 0.5) / cells
        u[a] = (k[a] + s) / cells                                   # on face f of voxel k
        h = _hit(u.astype(np.float32), normal)
        got = host.pick_face(h, (floats, ints))
        assert got.dtype == np.int32 and got.tolist() == [5, 9, 12, f]
        assert np.array_equal(got[:3], host.pick_grid_voxel(h, (floats, ints), 0))
    mid = ((k + 0.5) / cells).astype(np.float32)
    for bad in (_hit(mid, (0.6, 0.8, 0.0)), _hit(mid, (0, 0, 0)), _hit(mid, (1, 1, 0)), _hit(mid, (0, 2, 0)), _hit(mid, (0, 0, 0.5)),
                _hit(mid, (1, 0, 0), status=rt.RAY_MISS), _hit(mid, (1, 0, 0), fresh=0),
                _hit((1.5, 0.5, 0.5), (1, 0, 0))):                  # a non-axis normal, a miss, a stale record, outside the octree
        with pytest.raises(ValueError):
            host.pick_face(bad, (floats, ints))
