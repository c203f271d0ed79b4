"""Surface extraction without a GPU: the entry points are exported and bound, the Python struct layouts are the header's, the
kernels of tdt_surface.hip cross-compile without scratch or spills, the wrapper checks its arguments, the numpy model the GPU
tests compare against (tests/surface_model.py) keeps the invariants and closed forms of the definition, the host functions
(tdt_quads_to_mesh, tdt_ply_mesh_write) equal the model and round-trip through the PLY reader, and voxelising the extracted
surface gives back the dilated solid."""
import ctypes
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

import fill_model as fm
import mesh_model as mm
import morph_model
import surface_model as sm
from test_gpu_connect import block
from tdt4230_project_raytracing_amd import host, rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = sm.UNIT
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]                   # (merge, by_material)


def test_surface_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    assert hasattr(L, "tdt_octree_extract_surface")
    assert "tdt_octree_extract_surface" in {n for n, _, _ in rt.SYMBOLS}
    assert callable(rt.Context.octree_extract_surface)
    H = host.lib()
    for n in ("tdt_quads_to_mesh", "tdt_ply_mesh_write"):
        assert hasattr(H, n), n
    assert callable(host.quads_to_mesh) and callable(host.ply_mesh_write)


def test_surface_structs_match_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    for name, cls, size in (("tdt_surface", rt.Surface, 8), ("tdt_quad", rt.Quad, 32)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"int32_t\s+(\w+)(?:\[(\d+)\])?;", body)
        assert [f for f, _ in fields] == [f[0] for f in cls._fields_]
        offset = 0
        for (field, count), (_, ctype) in zip(fields, cls._fields_):
            assert getattr(cls, field).offset == offset, field
            assert ctypes.sizeof(ctype) == 4 * int(count or 1), field
            offset += 4 * int(count or 1)
        assert ctypes.sizeof(cls) == size == offset
        assert len(re.findall(r"sizeof\(%s\) == %d" % (name, size), text)) == 2      # C++ and C
    assert [f[0] for f in rt.Surface._fields_] == ["merge", "by_material"]
    assert [f[0] for f in rt.Quad._fields_] == ["face", "material", "origin", "size", "pad"]


def test_surface_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_surface.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"surface_probe_kernel", "surface_bounds_kernel", "surface_emit_kernel", "surface_head_flags_kernel",
            "surface_starts_kernel", "surface_runs_kernel", "surface_quads_kernel"} <= names
    # the keys kernel is the list layer's (resources: test_bitvol_api.py)
    shared = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in kernel_resources.collect("tdt_voxlist.hip")}
    assert "voxlist_keys_kernel" in shared and "surface_keys_kernel" not in names
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


def test_python_wrapper_argument_checks():
    s = rt.Context._surface(True, False)
    assert (s.merge, s.by_material) == (1, 0)
    assert rt.Context._surface(7, -3).merge == 7                              # the ranges are the library's to check
    for bad in (lambda: rt.Context._surface(0.5, 1), lambda: rt.Context._surface(1, 2 ** 31), lambda: rt.Context._surface(-2 ** 31 - 1, 0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        host.quads_to_mesh(np.zeros((1, 8), np.float32))


# ---- the model against its invariants ----------------------------------------------------------------------------------------
def random_grid(rng, depth, density, materials=3):
    n = 1 << depth
    occ = rng.random((n, n, n)) < density
    return sm.grid_voxels(occ, rng.integers(1, 1 + materials, (n, n, n)))


def exposed_faces_per_voxel(V, depth):
    """{(f, x, y, z)} counted voxel by voxel from a set of positions: shares nothing with the model's array code."""
    n = 1 << depth
    have = {tuple(p) for p in V[:, :3].tolist()}
    out = set()
    for x, y, z in have:
        for f in range(6):
            q = [x, y, z]
            q[f >> 1] += 1 if f & 1 else -1
            if min(q) < 0 or max(q) >= n or tuple(q) not in have:
                out.add((f, x, y, z))
    return out


def unit_faces(Q):
    """Every quad rasterised back to the unit faces (f, voxel x, y, z) it covers, with repetitions."""
    out = []
    for q in np.asarray(Q).tolist():
        a, s, u, v = sm.axes(q[0])
        for du in range(q[5]):
            for dv in range(q[6]):
                p = q[2:5]
                p[a] -= s                                                  # back from the plane to the voxel's own coordinate
                p[u] += du
                p[v] += dv
                out.append((q[0], *p))
                p[a] += s
                p[u] -= du
                p[v] -= dv
    return out


def signed_volume6(vertices, triangles):
    """Sum over triangles of a . (b x c), in Python integers: six times the enclosed volume."""
    total = 0
    v = vertices.tolist()
    for i, j, k in triangles.tolist():
        a, b, c = v[i], v[j], v[k]
        total += (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))
    return total


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_model_keeps_the_invariants_of_the_definition(depth):
    rng = np.random.default_rng(40 + depth)
    for density in (0.2, 0.5, 0.8):
        for _ in range(3 if depth < 4 else 1):
            V = random_grid(rng, depth, density)
            want = exposed_faces_per_voxel(V, depth)
            assert int(sm.exposed(V, depth).sum()) == len(want)
            mat = {tuple(p[:3]): p[3] for p in V.tolist()}
            for merge, by_material in MODES:
                Q = sm.quads(V, depth, merge, by_material)
                assert np.array_equal(Q, sm.quads_loop(V, depth, merge, by_material)), (density, merge, by_material)
                assert int((Q[:, 5] * Q[:, 6]).sum()) == len(want)
                got = unit_faces(Q)
                assert len(got) == len(want) and set(got) == want             # each exposed face exactly once
                if by_material:                                                # and under its own voxel's material
                    for q in Q.tolist():
                        assert {mat[p[1:]] for p in unit_faces([q])} == {q[1]}
                else:
                    assert not Q[:, 1].any()
                order = [tuple(q) for q in np.stack([Q[:, 0], Q[np.arange(len(Q)), 2 + (Q[:, 0] >> 1)] - (Q[:, 0] & 1),
                                                     Q[np.arange(len(Q)), 2 + ((Q[:, 0] >> 1) + 1) % 3],
                                                     Q[np.arange(len(Q)), 2 + ((Q[:, 0] >> 1) + 2) % 3]], 1).tolist()]
                assert order == sorted(order) and len(set(order)) == len(order)   # by face, w, u0, v0
                vert, tri, tm = sm.quads_to_mesh(Q)
                assert signed_volume6(vert, tri) == 6 * len(V) * U ** 3
                assert np.array_equal(tm, np.repeat(Q[:, 1], 2))
                if not merge:
                    edges = Counter()
                    for t in tri.tolist():
                        for e in range(3):
                            edges[(t[e], t[(e + 1) % 3])] += 1
                    assert all(edges[(b, a)] == c for (a, b), c in edges.items())


def test_sparse_occupancy_path_equals_the_dense_one(monkeypatch):
    rng = np.random.default_rng(5)
    V = random_grid(rng, 4, 0.5)
    dense = sm.exposed(V, 4)
    monkeypatch.setattr(sm, "DENSE_DEPTH", 0)
    assert np.array_equal(sm.exposed(V, 4), dense)


# ---- closed forms ------------------------------------------------------------------------------------------------------------
def test_closed_forms():
    one = np.array([[2, 3, 1, 9]], np.int32)
    Q = sm.quads(one, 2)
    assert len(Q) == 6 and (Q[:, 5:7] == 1).all() and (Q[:, 1] == 9).all()
    assert Q[:, 2:5].tolist() == [[2, 3, 1], [3, 3, 1], [2, 3, 1], [2, 4, 1], [2, 3, 1], [2, 3, 2]]
    full = block((0, 0, 0), (3, 3, 3), 5)
    Q = sm.quads(full, 2)
    assert len(Q) == 6 and (Q[:, 5:7] == 4).all()
    assert Q[:, 2:5].tolist() == [[0, 0, 0], [4, 0, 0], [0, 0, 0], [0, 4, 0], [0, 0, 0], [0, 0, 4]]
    assert len(sm.quads(full, 2, merge=False)) == 6 * 16
    chk = block((0, 0, 0), (7, 7, 7), 4)
    chk = sm.grid_voxels(fm.grid_of(chk[(chk[:, :3].sum(1) % 2) == 0], 3) > 0)
    for merge, by_material in MODES:
        assert len(sm.quads(chk, 3, merge, by_material)) == 6 * len(chk)      # nothing merges
    # two materials split along x in a 4 x 2 x 2 bar: the -x / +x caps are one quad each; the four long sides are cut at the
    # material boundary with by_material (2 + 4 * 2 = 10) and whole without it (6)
    bar = np.concatenate([block((0, 0, 0), (1, 1, 1), 1), block((2, 0, 0), (3, 1, 1), 2)])
    assert len(sm.quads(bar, 2, True, True)) == 10 and len(sm.quads(bar, 2, True, False)) == 6
    assert sorted(sm.quads(bar, 2, True, True)[:, 1].tolist()) == [1] * 5 + [2] * 5
    # three rows at one (w, u0) on consecutive v whose runs end at u1 = 5, 7, 5: the +x face (u = y, v = z) of voxels x = 0
    rows = np.concatenate([block((0, 0, 0), (0, 5, 0)), block((0, 0, 1), (0, 7, 1)), block((0, 0, 2), (0, 5, 2))])
    Q = sm.quads(rows, 3)
    Q = Q[Q[:, 0] == 1]
    assert Q[:, 2:7].tolist() == [[1, 0, 0, 6, 1], [1, 0, 1, 8, 1], [1, 0, 2, 6, 1]]      # rows 1 and 3 share u1 but are not adjacent
    assert len(sm.quads(np.zeros((0, 4), np.int32), 3)) == 0


def test_mask_cuts_quads_at_the_mask_not_at_a_run():
    plate = block((0, 0, 3), (7, 7, 3), 2)
    Q = sm.quads(plate, 3, regions=rt.box((0, 0, 0), (4, 7, 7)))
    top = Q[Q[:, 0] == 5]
    assert top[:, 2:7].tolist() == [[0, 0, 4, 5, 8]]                          # +z: u = x, v = y: x 0..4 only
    assert not (Q[:, 0] == 1).any()                                            # the +x faces at x = 7 lie outside the mask
    assert len(sm.quads(plate, 3, regions=[])) == 0


# ---- the host functions against the model --------------------------------------------------------------------------------------
def test_host_quads_to_mesh_equals_the_model():
    rng = np.random.default_rng(77)
    for depth, merge, by_material in ((2, 1, 1), (3, 0, 1), (4, 1, 0), (4, 1, 1)):
        Q = sm.quads(random_grid(rng, depth, 0.45), depth, merge, by_material)
        got, want = host.quads_to_mesh(Q), sm.quads_to_mesh(Q)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
        v = got[0]
        assert len(np.unique(v, axis=0)) == len(v) and (np.lexsort((v[:, 2], v[:, 1], v[:, 0])) == np.arange(len(v))).all()
    v, t, m = host.quads_to_mesh(np.zeros((0, 8), np.int32))
    assert v.shape == (0, 3) and t.shape == (0, 3) and m.shape == (0,)
    # depth 10: the far corner of the lattice
    Q = sm.quads(np.array([[1023, 1023, 1023, 3]], np.int32), 10)
    got, want = host.quads_to_mesh(Q), sm.quads_to_mesh(Q)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[0].max() == 1024 * U


def test_host_count_queries_and_small_buffers_write_nothing():
    L = host.lib()
    Q = np.ascontiguousarray(sm.quads(block((1, 1, 1), (2, 2, 1), 4), 2))
    want_v, want_t, _ = sm.quads_to_mesh(Q)
    host.quads_to_mesh(Q)                                                     # sets the argtypes
    nv, nt = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.tdt_quads_to_mesh(Q.ctypes.data, len(Q), None, 0, ctypes.byref(nv), None, None, 0, ctypes.byref(nt)) == 0
    assert (nv.value, nt.value) == (len(want_v), len(want_t)) == (8, 12)                   # a 2 x 2 x 1 box: 8 corners, 6 quads
    v, t, m = np.full((8, 3), -7, np.int32), np.full((12, 3), 9999, np.uint32), np.full(12, -7, np.int32)
    for cap_v, cap_t in ((7, 12), (8, 11)):
        nv, nt = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert L.tdt_quads_to_mesh(Q.ctypes.data, len(Q), v.ctypes.data, cap_v, ctypes.byref(nv), t.ctypes.data, m.ctypes.data, cap_t,
                                   ctypes.byref(nt)) == 0x0501
        assert (nv.value, nt.value) == (8, 12) and (v == -7).all() and (t == 9999).all() and (m == -7).all()
    assert L.tdt_quads_to_mesh(Q.ctypes.data, len(Q), v.ctypes.data, 8, ctypes.byref(nv), t.ctypes.data, None, 12, ctypes.byref(nt)) == 0
    assert np.array_equal(v, want_v) and np.array_equal(t, want_t) and (m == -7).all()     # materials are optional
    for bad in ([[6, 1, 0, 0, 0, 1, 1, 0]], [[0, 1, 0, 0, 0, 0, 1, 0]], [[0, 1, -1, 0, 0, 1, 1, 0]], [[3, 1, 0, 0, 4096, 1, 1, 0]]):
        with pytest.raises(RuntimeError):
            host.quads_to_mesh(np.array(bad, np.int32))
    # the PLY writer
    text = host.ply_mesh_write(want_v, want_t)
    n = ctypes.c_size_t(0)
    assert L.tdt_ply_mesh_write(want_v.ctypes.data, len(want_v), want_t.ctypes.data, len(want_t), None, 0, ctypes.byref(n)) == 0
    assert n.value == len(text)
    buf = ctypes.create_string_buffer(b"\x55" * len(text), len(text))
    n = ctypes.c_size_t(0)
    assert L.tdt_ply_mesh_write(want_v.ctypes.data, len(want_v), want_t.ctypes.data, len(want_t), buf, len(text) - 1, ctypes.byref(n)) == 0x0501
    assert n.value == len(text) and buf.raw == b"\x55" * len(text)
    with pytest.raises(RuntimeError):
        host.ply_mesh_write(want_v, np.array([[0, 1, 8]], np.uint32))           # an index past the vertices


def test_ply_round_trip_returns_the_mesh():
    rng = np.random.default_rng(3)
    Q = sm.quads(random_grid(rng, 3, 0.4), 3)
    v, t, _ = host.quads_to_mesh(Q)
    for verts, tris in ((v, t), (np.array([[-64 * 4096, 1, 33], [5, -63, 64 * 4096], [96, 48, 16385]], np.int32), np.array([[0, 1, 2]], np.uint32)),
                        (np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32))):
        text = host.ply_mesh_write(verts, tris)
        assert text.startswith(b"ply\nformat ascii 1.0\n") and b"e" not in text.split(b"end_header\n")[1]   # plain decimals
        back = host.PlyMesh(text)
        assert back.vertices.shape == verts.shape and back.triangles.shape == tris.shape
        assert np.array_equal(host.mesh_quantize(back.vertices), verts) and np.array_equal(back.triangles, tris)
    assert b"\n0.015625 -0.984375 4096\n" in host.ply_mesh_write(np.array([[1, -63, 64 * 4096]], np.int32), np.zeros((0, 3), np.uint32))


# ---- the round trip on the models alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", [0, 1])
@pytest.mark.parametrize("depth", [3, 4])
def test_voxelising_the_surface_gives_the_dilated_solid(depth, merge):
    """Closed-triangle coverage marks every voxel whose closed cube touches the boundary of V — the 26-dilation's new voxels and
    V's own surface voxels — and the fill closes what they enclose: V's interior."""
    n = 1 << depth
    rng = np.random.default_rng(10 * depth + merge)
    occ = np.zeros((n, n, n), bool)
    occ[1:-1, 1:-1, 1:-1] = rng.random((n - 2,) * 3) < 0.5                   # strictly inside the grid
    V = sm.grid_voxels(occ)
    vert, tri, _ = sm.quads_to_mesh(sm.quads(V, depth, merge, by_material=False))
    S = mm.voxelize_many(vert, tri, depth)
    got = fm.filled(S, depth)
    want = fm.filled(morph_model.morph(V, depth, rt.MORPH_DILATE, 1, 26), depth)
    assert len(V) and np.array_equal(fm.keys(got[:, :3]), fm.keys(want[:, :3]))
