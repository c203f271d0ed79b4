"""tests/tree_model.py is what the depth-10 scenes of the build matrix come from, so the oracle's input there does not depend on
the GPU builder: its build_cells must write the host builder's bytes (csrc/host_scene.cpp build_octree), and its scene payloads
those of Octree::init_global_buffers."""
import numpy as np
import pytest

import tree_model
from octree_util import expand_cells
from tdt4230_project_raytracing_amd import host

GENERATED = [(kind, depth) for kind in (host.SCENE_HASH_GRID, host.SCENE_TERRAIN, host.SCENE_SHELLS) for depth in (4, 7, 9)
             if (kind, depth) != (host.SCENE_HASH_GRID, 9)]      # (the depth-9 hash grid needs more than 2^21 cells: it cannot be generated)


def _same(scene):
    d = scene.max_depth
    cells = tree_model.build_cells(expand_cells(scene.blobs[0], d), d)
    assert cells.dtype == np.uint32 and cells.tobytes() == scene.blobs[0].tobytes()


@pytest.mark.parametrize("config", [1, 2, 3])
def test_builder_writes_the_host_builders_bytes_for_the_configs(config):
    _same(host.Scene.config(config))


@pytest.mark.parametrize("kind,depth", GENERATED)
def test_builder_writes_the_host_builders_bytes_for_generated_scenes(kind, depth):
    _same(host.Scene.generate(kind, depth, 1 << 20, 256, 7))


def test_depth_10_round_trip_with_voxels_in_all_eight_corners():
    rng = np.random.default_rng(10)
    n = 1 << 10
    corners = np.array([[x, y, z] for x in (0, n - 1) for y in (0, n - 1) for z in (0, n - 1)], np.int64)
    block = np.stack(np.meshgrid(*([np.arange(8)] * 3), indexing="ij"), axis=-1).reshape(-1, 3) + 512      # a level-7 block: one LEAF
    loose = rng.integers(0, n, size=(4000, 3))
    slab = np.stack(np.meshgrid(np.arange(100, 164), [37], np.arange(900, 964), indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = np.unique(np.concatenate([corners, block, loose, slab]), axis=0)
    mat = rng.integers(1, 21, size=len(xyz))
    mat[(xyz >= 512).all(axis=1) & (xyz < 520).all(axis=1)] = 5
    vox = np.concatenate([xyz, mat[:, None]], axis=1).astype(np.int32)
    cells = tree_model.build_cells(vox, 10)
    back = expand_cells(cells, 10)
    order = lambda v: v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]
    assert np.array_equal(order(back), order(vox))
    assert tree_model.parents_at_level(cells, 9) > 0 and tree_model.parents_at_level(cells, 10) == 0
    c = cells.reshape(-1, 8, 2)
    assert ((c[..., 1] == tree_model.LEAF) & (c[..., 0] == 4)).sum() >= 1                                  # the block merged
    # breadth-first and compact: the PARENT values are 1, 2, 3, ... in node order
    par = c[..., 0][c[..., 1] == tree_model.PARENT]
    assert np.array_equal(par, np.arange(1, len(c), dtype=np.uint32))


def test_an_empty_voxel_list_is_one_empty_cell():
    assert np.array_equal(tree_model.build_cells(np.zeros((0, 4), np.int32), 5), np.zeros(16, np.uint32))


def test_scene_payloads_are_init_global_buffers():
    """octree.rs:44-50, 76-81: {min_point, 0, scale, 1 / scale, 1 / cell_count as f32} and {max_depth, max_iter, cell_count} — the
    host's own scenes come back bit for bit, and a count that is not a power of two gets f32(1) / f32(count)."""
    for like in (host.Scene.config(2), host.Scene.demo()):
        s = tree_model.scene_from_cells(like.blobs[0], like.max_depth, like.cell_count, like)
        for slot in host.SLOTS:
            assert s.blobs[slot].dtype == like.blobs[slot].dtype and s.blobs[slot].tobytes() == like.blobs[slot].tobytes(), slot
    like = host.Scene.config(1)
    s = tree_model.scene_from_cells(like.blobs[0], 10, 1000003, like, min_point=(0.75, -1.5, 0.25))
    assert s.blobs[6].view(np.uint32).tolist() == np.array([0.75, -1.5, 0.25, 0.0, 1.0, 1.0, np.float32(1.0) / np.float32(1000003)], np.float32).view(np.uint32).tolist()
    assert s.blobs[7].tolist() == [10, like.max_iter, 1000003]
    same = host.scene_with_cell_count(like, 1000003)
    assert s.blobs[6][6] == same.blobs[6][6]
    neg = tree_model.with_corner(s, np.array([0x80000000, 0, 0x3F800000], np.uint32).view(np.float32))
    assert neg.blobs[6][:3].view(np.uint32).tolist() == [0x80000000, 0, 0x3F800000]
