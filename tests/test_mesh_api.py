"""Triangle-mesh voxelisation without a GPU: the entry points are exported and bound, the Python tdt_mesh layout is the
header's, the kernels of tdt_mesh.hip cross-compile without scratch or spills, the numpy model the GPU tests compare against
equals exact rational clipping and the closed forms of the definition, the host functions (quantise, fit, the PLY mesh reader)
equal their numpy restatements, and the wrapper checks its arguments."""
import ctypes
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import mesh_model as mm
from tdt4230_project_raytracing_amd import host, rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdt_voxelize_triangles", "tdt_octree_edit_triangles")
U = mm.UNIT


def test_mesh_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    H = host.lib()
    for n in ("tdt_mesh_quantize", "tdt_mesh_fit", "tdt_ply_mesh_parse", "tdt_ply_mesh_destroy", "tdt_ply_mesh_info", "tdt_ply_mesh_vertices",
              "tdt_ply_mesh_triangles"):
        assert hasattr(H, n), n


def test_mesh_struct_and_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_mesh \{(.*?)\} tdt_mesh;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for kind, names in re.findall(r"((?:const\s+)?u?int32_t\s*\*?)\s*([^;]+);", body):
        pointer = "*" in kind or names.strip().startswith("*")
        base = "uint32_t" if "uint32_t" in kind else "int32_t"
        for f in names.split(","):
            fields.append((base, pointer, f.strip().lstrip("*")))
    assert [f[2] for f in fields] == [f[0] for f in rt.Mesh._fields_] == ["vertices", "triangles", "materials", "n_vertices", "n_triangles",
                                                                        "material", "pad"]
    offset = 0
    for base, pointer, name in fields:
        ctype = dict(rt.Mesh._fields_)[name]
        assert getattr(rt.Mesh, name).offset == offset, name
        assert ctype is (ctypes.c_void_p if pointer else ctypes.c_uint32 if base == "uint32_t" else ctypes.c_int32), name
        offset += 8 if pointer else 4
    assert offset == ctypes.sizeof(rt.Mesh) == 40
    assert len(re.findall(r"sizeof\(tdt_mesh\) == 40", text)) == 2           # C++ and C
    assert re.search(r"#define TDT_MESH_FRAC 6\b", text) and rt.MESH_FRAC == mm.FRAC == 6
    assert re.search(r"#define TDT_MESH_COORD_MAX \(1 << 18\)", text) and rt.MESH_COORD_MAX == mm.COORD_MAX == 1 << 18


def test_mesh_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_mesh.hip")
    names = {re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows}
    assert {"mesh_setup_kernel", "mesh_tiles_kernel", "mesh_pairs_kernel", "mesh_voxels_kernel", "mesh_last_kernel", "mesh_emit_kernel"} <= names
    assert sum("mesh_voxels_kernel<" in r["name"] for r in rows) == 2
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]


# ---- the model against exact rational clipping -------------------------------------------------------------------------------
def clip_nonempty(tri, lo, hi):
    """Sutherland-Hodgman of the closed triangle (possibly a segment or a point) against the closed box [lo, hi], in rationals: is
    anything left?  Clipping a convex polygon by a closed half-space keeps exactly its points inside it, degenerate ones too."""
    poly = [tuple(Fraction(int(c)) for c in p) for p in tri]
    for axis in range(3):
        for bound, sign in ((lo[axis], 1), (hi[axis], -1)):
            def inside(p):
                return sign * (p[axis] - bound) >= 0
            out = []
            for i, q in enumerate(poly):
                p = poly[i - 1]
                if inside(q):
                    if not inside(p):
                        s = (bound - p[axis]) / (q[axis] - p[axis])
                        out.append(tuple(p[k] + s * (q[k] - p[k]) for k in range(3)))
                    out.append(q)
                elif inside(p):
                    s = (bound - p[axis]) / (q[axis] - p[axis])
                    out.append(tuple(p[k] + s * (q[k] - p[k]) for k in range(3)))
            poly = out
            if not poly:
                return False
    return True


def test_model_equals_exact_rational_clipping():
    depth, n = 2, 4
    rng = np.random.default_rng(13)
    v, t, kinds = mm.random_triangles(rng, 306, n)
    assert set(kinds) == set(mm.KINDS) and len(t) >= 300
    vox = mm.grid(np.zeros(3, np.int64), np.full(3, n - 1, np.int64))
    hits = 0
    per_kind = {k: 0 for k in mm.KINDS}
    for idx, kind in zip(t, kinds):
        tri = v[idx].astype(np.int64)
        got = {tuple(p) for p in mm.covered(tri, depth)}
        want = {tuple(p) for p in vox if clip_nonempty(tri, p * U, p * U + U)}
        assert got == want, (kind, tri.tolist())
        assert np.array_equal(mm.overlap(tri, vox * U, U), [tuple(p) in want for p in vox])      # the flat test too
        hits += len(want)
        per_kind[kind] += len(want)
    assert 0 < hits < len(t) * len(vox)
    assert all(per_kind.values()), per_kind


def test_batched_model_equals_the_per_triangle_model():
    """voxelize_many (whole batches of (triangle, box voxel) pairs; tools/mesh_time.py checks 10^6-triangle meshes with it) against
    voxelize, with the hierarchical path forced for the larger triangles."""
    rng = np.random.default_rng(21)
    for depth in (3, 5):
        v, t, _ = mm.random_triangles(rng, 120, 1 << depth)
        mats = rng.integers(1, 255, len(t))
        want = mm.voxelize(v, t, depth, mats)
        assert len(want) and np.array_equal(mm.voxelize_many(v, t, depth, mats, flat_limit=300, chunk=1000), want)
        assert np.array_equal(mm.voxelize_many(v, t, depth, None, 8), mm.voxelize(v, t, depth, None, 8))


def test_closed_forms():
    tri = np.array([[0, 1, 2]], np.uint32)
    corner = np.full((3, 3), 2 * U, np.int32)
    got = mm.voxelize(corner, tri, 2, material=4)
    assert {tuple(p) for p in got[:, :3]} == {(x, y, z) for x in (1, 2) for y in (1, 2) for z in (1, 2)} and set(got[:, 3]) == {5}
    assert mm.voxelize(corner + U // 2, tri, 2).tolist() == [[2, 2, 2, 1]]
    # an axis-aligned rectangle in the boundary plane y = 2 voxels: exactly the two slabs next to it
    rect = np.array([[0, 2 * U, 0], [4 * U, 2 * U, 0], [4 * U, 2 * U, 4 * U], [0, 2 * U, 4 * U]], np.int32)
    got = mm.voxelize(rect, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), 2)
    assert {tuple(p) for p in got[:, :3]} == {(x, y, z) for x in range(4) for y in (1, 2) for z in range(4)}
    # on the grid's low face only the inside layer exists; off the grid: nothing
    rect[:, 1] = 0
    got = mm.voxelize(rect, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), 2)
    assert {tuple(p) for p in got[:, :3]} == {(x, 0, z) for x in range(4) for z in range(4)}
    assert len(mm.voxelize(corner + 9 * U, tri, 2)) == 0
    # the highest covering triangle gives the material, and the list is in Morton order
    two = mm.voxelize(np.concatenate([corner, corner]), np.array([[0, 1, 2], [3, 4, 5]], np.uint32), 2, materials=[9, 3])
    assert set(two[:, 3]) == {3}
    key = mm.morton(two[:, :3])
    assert (key[1:] > key[:-1]).all()


# ---- the host functions ------------------------------------------------------------------------------------------------------
def test_quantize_equals_numpy_ties_included():
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-60, 60, (500, 3)).astype(np.float32)
    ties = (np.arange(-40, 41, dtype=np.float64)[:, None] + 0.5) / 64.0 * np.ones(3)      # x * 64 = k + 0.5: ties to even
    xyz = np.concatenate([xyz, ties.astype(np.float32)])
    assert np.array_equal(ties.astype(np.float32).astype(np.float64), ties)                # exactly representable
    got = host.mesh_quantize(xyz)
    assert got.dtype == np.int32 and np.array_equal(got, mm.quantize(xyz))
    assert np.array_equal(got[500:, 0], np.rint(np.arange(-40, 41) + 0.5).astype(np.int64)) and (got[500:, 0] % 2 == 0).all()
    for scale, off in ((3.7, (0.1, -2.25, 9.0)), (0.013, (512.0, 100.5, 0.0))):
        assert np.array_equal(host.mesh_quantize(xyz, scale, off), mm.quantize(xyz, scale, off))
    assert host.mesh_quantize(np.array([[4096.0, -4096.0, 0.0]], np.float32)).tolist() == [[1 << 18, -(1 << 18), 0]]
    for bad in ([[4096.01, 0, 0]], [[0, -5000.0, 0]], [[np.inf, 0, 0]], [[0, 0, np.nan]]):
        with pytest.raises(ValueError, match="0x501"):
            host.mesh_quantize(np.array(bad, np.float32))
    with pytest.raises(ValueError):
        host.mesh_quantize(xyz, np.inf)
    assert host.mesh_quantize(np.zeros((0, 3), np.float32)).shape == (0, 3)


def test_fit_equals_numpy():
    rng = np.random.default_rng(4)
    for lo, hi in (((1, 1, 1), (62, 62, 62)), ((0, 0, 0), (1023, 1023, 1023)), ((5, 9, 2), (20, 11, 40))):
        xyz = (rng.normal(size=(40, 3)) * rng.uniform(0.1, 30, 3) + rng.uniform(-50, 50, 3)).astype(np.float32)
        scale, off = host.mesh_fit(xyz, lo, hi)
        want_s, want_o = mm.fit(xyz, lo, hi)
        assert scale == want_s and np.array_equal(off, want_o)
        p = xyz.astype(np.float64) * scale + off
        room = np.array(hi) + 1.0 - np.array(lo)
        assert (p.min(0) >= np.array(lo) - 1e-9).all() and (p.max(0) <= np.array(hi) + 1 + 1e-9).all()       # it fits
        assert np.isclose((p.max(0) - p.min(0)) / room, 1.0).any()                                       # and one edge spans the box
        assert np.allclose((p.max(0) + p.min(0)) * 0.5, (np.array(lo) + np.array(hi) + 1.0) * 0.5)        # centred
    # a flat mesh: the axes with an extent decide; a point: scale 1, centred
    flat = np.array([[0, 0, 0], [2, 0, 1], [1, 0, 3]], np.float32)
    scale, off = host.mesh_fit(flat, (0, 0, 0), (15, 15, 15))
    assert (scale, off.tolist()) == (mm.fit(flat, (0, 0, 0), (15, 15, 15))[0], mm.fit(flat, (0, 0, 0), (15, 15, 15))[1].tolist())
    assert scale == 16.0 / 3.0
    scale, off = host.mesh_fit(np.array([[7.5, 1, 2]], np.float32), (0, 0, 0), (15, 15, 15))
    assert scale == 1.0 and off.tolist() == [0.5, 7.0, 6.0]
    for bad in (lambda: host.mesh_fit(np.zeros((0, 3), np.float32), (0, 0, 0), (3, 3, 3)), lambda: host.mesh_fit(flat, (4, 0, 0), (3, 3, 3)),
                lambda: host.mesh_fit(np.array([[np.nan, 0, 0]], np.float32), (0, 0, 0), (3, 3, 3))):
        with pytest.raises(ValueError):
            bad()


CUBE_V = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
CUBE_F = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)]


def ply_text(verts=CUBE_V, faces=CUBE_F, eol="\n", fmt="ascii 1.0", extra=(), index_name="vertex_indices", count_type="uchar", index_type="int",
             coord_type="float"):
    head = ["ply", f"format {fmt}", "comment made by a test", f"element vertex {len(verts)}"]
    head += [f"property {coord_type} {a}" for a in "xyz"] + [f"property {t} {n}" for t, n in extra]
    head += [f"element face {len(faces)}", f"property list {count_type} {index_type} {index_name}", "end_header"]
    body = [" ".join(str(c) for c in v) for v in verts] + [" ".join(str(c) for c in (len(f),) + tuple(f)) for f in faces]
    return (eol.join(head + body) + eol).encode()


def test_ply_mesh_reader(tmp_path):
    want_t = np.array([(f[0], f[i], f[i + 1]) for f in CUBE_F for i in (1, 2)], np.uint32)
    for eol in ("\n", "\r\n"):
        path = tmp_path / f"cube{len(eol)}.ply"
        path.write_bytes(ply_text(eol=eol))
        m = host.PlyMesh(path.read_bytes())
        assert m.faces == 6 and m.triangles.shape == (12, 3) and np.array_equal(m.triangles, want_t)
        assert m.vertices.dtype == np.float32 and np.array_equal(m.vertices, np.array(CUBE_V, np.float32))
    # an extra vertex property (colours are skipped), the other spelling of the list, other scalar types, a pentagon
    verts = [v + (255, 0, 10, 0.5) for v in CUBE_V]
    extra = (("uchar", "red"), ("uchar", "green"), ("uchar", "blue"), ("float", "quality"))
    m = host.PlyMesh(ply_text(verts, CUBE_F + [(0, 1, 2, 6, 7)], extra=extra, index_name="vertex_index", count_type="uint8", index_type="uint32",
                              coord_type="double"))
    assert np.array_equal(m.vertices, np.array(CUBE_V, np.float32)) and m.faces == 7
    assert np.array_equal(m.triangles, np.concatenate([want_t, [(0, 1, 2), (0, 2, 6), (0, 6, 7)]]))
    m = host.PlyMesh(ply_text([(0.25, -1.5e1, 3)] * 3, [(0, 1, 2)]))
    assert m.vertices.tolist() == [[0.25, -15.0, 3.0]] * 3
    # errors, each with a message
    good = ply_text()
    cases = {
        "binary": ply_text(fmt="binary_little_endian 1.0"),
        "two indices": ply_text(faces=[(0, 1)]),
        "index too large": ply_text(faces=[(0, 1, 8)]),
        "negative index": ply_text(faces=[(0, -1, 2)]),
        "truncated face": good[: good.rindex(b"3 0 4 7")] + b"3 0\n",
        "truncated vertices": ply_text(verts=CUBE_V[:5], faces=[]).replace(b"element vertex 5", b"element vertex 9"),
        "trailing data": good + b"1 2 3\n",
        "not ply": b"plx\n" + good[4:],
        "no face element": good.replace(b"element face 6\nproperty list uchar int vertex_indices\n", b""),
        "int coordinates": ply_text(coord_type="int"),
        "y before x": good.replace(b"property float x\nproperty float y", b"property float y\nproperty float x"),
        "face list type": ply_text(index_type="float"),
        "another element": good.replace(b"end_header", b"element edge 0\nend_header"),
        "not a number": good.replace(b"1 1 0\n", b"1 one 0\n", 1),
        "no end_header": good[: good.index(b"end_header")],
    }
    for name, data in cases.items():
        with pytest.raises(ValueError, match="0x501") as e:
            host.PlyMesh(data)
        assert len(str(e.value)) > 12, name


# ---- the wrapper's argument checks -------------------------------------------------------------------------------------------
def test_python_wrapper_argument_checks():
    v = np.zeros((3, 3), np.int32)
    t = np.array([[0, 1, 2]], np.uint32)
    mesh, keep = rt._mesh(v, t, [5], 3)
    assert (mesh.n_vertices, mesh.n_triangles, mesh.material) == (3, 1, 3) and mesh.vertices == keep[0].ctypes.data
    assert mesh.materials == keep[2].ctypes.data and keep[2].dtype == np.int32
    empty, _ = rt._mesh(np.zeros((0, 3)).astype(np.int32), np.zeros((0, 3), np.uint32), None, 0)
    assert (empty.vertices, empty.triangles, empty.materials, empty.n_triangles) == (None, None, None, 0)
    for bad in (lambda: rt._mesh(v.astype(np.float32), t, None, 0),          # float vertices: quantise first
                lambda: rt._mesh(v, np.array([[0, 1, -1]]), None, 0),        # an index that would wrap
                lambda: rt._mesh(v, np.array([[0, 1, 2 ** 32]]), None, 0),
                lambda: rt._mesh(v.astype(np.int64) + 2 ** 40, t, None, 0),
                lambda: rt._mesh(v, t, [1, 2], 0),                           # one material per triangle
                lambda: rt._mesh(v, t, [1.5], 0),
                lambda: rt._mesh(v[:, :2], t, None, 0),
                lambda: rt._mesh(v, t, None, 2 ** 31),
                lambda: rt._mesh(v, t, None, True)):
        with pytest.raises(ValueError):
            bad()
