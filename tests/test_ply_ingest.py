"""Next row §8f-1: the PLY point loader (ply_point_loader.rs:102-319) restated, and the octree build
the reference never wrote.  PARITY UNPINNED for the loader (no Rust toolchain to run it): expected
values below are derived by hand from the reference source for its own 3x3x3 model.  The reference's two model files are pinned
by their SHA-256 and its render of the large one, both recorded by oracle/make_goldens.py --live (tests/golden/live/)."""
import hashlib
import json
import os

import numpy as np
import pytest

from tdt4230_project_raytracing_amd import host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def model_sha256(name):
    z = np.load(os.path.join(GOLDEN, "live", "reference_live.npz"))
    return json.loads(str(z["meta"]))["models_sha256"][name]


HEADER = ["ply", "format ascii 1.0", "comment : MagicaVoxel @ Ephtracy", "element vertex {n}", "property float x",
          "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
          "end_header"]


def cube_edges_ply(eol):
    """The reference's assets/models/3x3x3_point.ply regenerated: corners and edges of a 3x3x3 cube (20 voxels)."""
    vox = [(x, y, z) for z in (0, 1, 2) for y in (-1, 0, 1) for x in (-1, 0, 1)
           if (x == 0) + (y == 0) + (z == 1) <= 1]
    lines = [h.format(n=len(vox)) for h in HEADER] + [f"{x} {y} {z} 153 153 255" for x, y, z in vox]
    return (eol.join(lines) + eol).encode(), vox


def test_regenerated_model_is_the_reference_file():
    assert hashlib.sha256(cube_edges_ply("\n")[0]).hexdigest() == model_sha256("3x3x3_point.ply")


def test_loader_content():
    data, vox = cube_edges_ply("\r\n")
    p = host.Ply(data, strict_crlf=True)
    assert p.header_vertex == 20 and len(p.positions) == 20
    assert p.positions.tolist() == [list(v) for v in vox]
    assert p.min_point == [-1, -1, 0]                                   # :221,:267-276
    k = host.cantor_pair(153, 153, 255)
    assert (p.albedo_keys == k).all()
    # the key is recomputed and inserted after EVERY property (:300-307): partial colours pollute the palette
    assert p.albedos == {host.cantor_pair(0, 0, 0): (0, 0, 0), host.cantor_pair(153, 0, 0): (153, 0, 0),
                         host.cantor_pair(153, 153, 0): (153, 153, 0), k: (153, 153, 255)}
    assert host.cantor_pair(0, 0, 0) == 0 and host.cantor_pair(255, 255, 255) == 0xFFFFFFFF   # f64 -> u32 saturates


def test_strict_grammar_is_crlf_only():
    lf, _ = cube_edges_ply("\n")
    with pytest.raises(RuntimeError) as e:
        host.Ply(lf, strict_crlf=True)                                  # "ply\r\n" expected at :121
    assert "Unexpected character at offset '3', State: ReadHeader(Ply)" in str(e.value)
    p = host.Ply(lf, strict_crlf=False)
    assert len(p.positions) == 20


@pytest.mark.parametrize("mutate,msg", [
    (lambda s: s.replace(b"format ascii 1.0", b"format binary 1.0"), "Unexpected format"),
    (lambda s: s.replace(b"property float x", b"property double x"), "Unexpected type"),
    (lambda s: s.replace(b"property float x", b"property float w"), "Unexpected variable"),
    (lambda s: s.replace(b"element vertex", b"element face  "), "Unexpected character"),
    (lambda s: s.replace(b"-1 -1 0 153", b"-1 -1.5 0 153"), "FloatParseError"),
    (lambda s: s.replace(b"153 153 255\r\n0 -1 0", b"153 300 255\r\n0 -1 0"), "FloatParseError"),
    (lambda s: s.replace(b"comment :", b"obj_info "), "header keyword"),
])
def test_loader_errors(mutate, msg):
    data, _ = cube_edges_ply("\r\n")
    with pytest.raises(RuntimeError) as e:
        host.Ply(mutate(data))
    assert msg in str(e.value)


def test_prefix_keyword_quirk():
    """expect() compares only the zipped length (:324-327): 'prop' passes for 'property'."""
    data, _ = cube_edges_ply("\r\n")
    quirky = data.replace(b"property float x", b"prop     float x")     # same byte offsets
    assert host.Ply(quirky).positions.shape == (20, 3)


def test_octree_from_ply(oracle):
    data, vox = cube_edges_ply("\r\n")
    scene = host.Ply(data).to_scene(max_iter=100)
    assert scene.max_depth == 2 and scene.counts["voxels"] == 20 and scene.counts["materials"] == 1
    assert scene.blobs[2].tolist() == [float(np.float32(153) / np.float32(255))] * 2 + [1.0]
    cells = scene.blobs[0].reshape(-1, 8, 2)
    assert set(np.unique(cells[..., 1])) <= {0, 1, 2} and (cells[..., 0][cells[..., 1] == 2] == 0).all()
    img = oracle.render(scene, host.camera_reference_pose(64, 64, 1, 2), threads=2)
    assert (img[..., 3] == 1).all() and (img[..., :3] != img[0, 0, :3]).any()    # the model is in view


def monument_ply():
    """The reference's assets/models/monu1_point.ply rebuilt from its vertex lines (tests/golden/live/monu1_point.npz) under the
    header of the 3x3x3 model; the render the reference shader made of it rides along."""
    z = np.load(os.path.join(GOLDEN, "live", "monu1_point.npz"))
    xyz, rgb = z["xyz"], z["rgb"]
    lines = [h.format(n=len(xyz)) for h in HEADER] + [f"{x} {y} {z_} {r} {g} {b}" for (x, y, z_), (r, g, b) in zip(xyz.tolist(), rgb.tolist())]
    return ("\n".join(lines) + "\n").encode(), z["image"]


def test_reference_monument_model(oracle):
    """The reference's large model (156 942 voxels): parsed, built, and the resulting octree rendered
    identically by the reference shader and the oracle."""
    data, ref = monument_ply()
    assert hashlib.sha256(data).hexdigest() == model_sha256("monu1_point.ply")
    p = host.Ply(data, strict_crlf=False)
    assert p.header_vertex == 156942 and len(p.positions) == 156942
    assert p.min_point == [-29, -52, 0]
    scene = p.to_scene(max_iter=256)
    assert scene.max_depth == 7 and scene.counts["voxels"] == 156942 and scene.counts["materials"] == 8
    cam = host.camera_reference_pose(128, 96, 2, 4)
    got = oracle.render(scene, cam, threads=8)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
