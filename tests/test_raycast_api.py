"""Ray queries without a GPU: the entry points are exported, the Python record layout is the header's, the query kernel
cross-compiles without scratch or spills, and the pick-to-edit arithmetic (tdt_pick_edit_delta) lands on the right cells."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from tdt4230_project_raytracing_amd import host, rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_entry_points_are_exported():
    L = ctypes.CDLL(rt.LIB_PATH)
    for n in ("tdt_raycast", "tdt_raycast_device", "tdt_pick_pixels"):
        assert hasattr(L, n), n
    assert hasattr(host.lib(), "tdt_pick_edit_delta")


def test_ray_hit_dtype_matches_the_header():
    text = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
    body = re.search(r"typedef struct tdt_ray_hit \{(.*?)\} tdt_ray_hit;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int32_t|uint32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    kinds = {"int32_t": "<i4", "uint32_t": "<u4", "float": "<f4"}
    offset = 0
    assert rt.RAY_HIT_DTYPE.itemsize == 64
    assert list(rt.RAY_HIT_DTYPE.names) == [f[1] for f in fields]
    for ctype, name, count in fields:
        dt, off = rt.RAY_HIT_DTYPE.fields[name][:2]
        assert off == offset, name
        base = dt.subdtype[0] if dt.subdtype else dt
        assert base == np.dtype(kinds[ctype]), name
        assert (dt.shape or (1,)) == ((int(count),) if count else (1,)), name
        offset += 4 * (int(count) if count else 1)
    assert offset == 64


def test_query_kernel_has_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = [r for r in kernel_resources.collect("tdt_query.hip") if r["name"].startswith("tdt::raycast_kernel")]
    assert len(rows) == 2                                     # the ray form and the pick form
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
        assert r["LDS Size [bytes/block]"] <= 64, r           # the one-entry escape table only


# ---- tdt_pick_edit_delta -------------------------------------------------------------------------------------------------
MIN = np.array([-0.5, -0.5, -1.0], np.float32)
NORMALS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def _octree(depth, scale=1.0, min_point=MIN):
    floats = np.array([min_point[0], min_point[1], min_point[2], 0.0, scale, 1.0 / scale, 1.0 / 100000.0], np.float32)
    return floats, np.array([depth, 100, 100000], np.int32)


def _hit(point, normal, status=rt.RAY_HIT, fresh=1):
    h = np.zeros(1, rt.RAY_HIT_DTYPE)
    h["status"] = status
    h["fresh_record"] = fresh
    h["front_face"] = 1
    h["point"] = np.asarray(point, np.float32)
    h["normal"] = np.asarray(normal, np.float32)
    return h


def _face_point(cell, normal, depth, scale, min_point, uv, nudge):
    """A point of the face of finest cell `cell` whose outward normal is `normal`, at in-face position uv, moved `nudge` ulps
    across the face (a traced hit point is a rounded value near the plane, on either side)."""
    g = 1 << depth
    n = np.asarray(normal)
    a = int(np.flatnonzero(n)[0])
    q = (np.asarray(cell, np.float64) + 0.5) / g
    q[a] = (cell[a] + (1 if n[a] > 0 else 0)) / g
    others = [i for i in range(3) if i != a]
    q[others[0]] = (cell[others[0]] + uv[0]) / g
    q[others[1]] = (cell[others[1]] + uv[1]) / g
    p = (q * scale + min_point.astype(np.float64)).astype(np.float32)
    for _ in range(abs(nudge)):
        p[a] = np.nextafter(p[a], np.float32(np.inf if nudge > 0 else -np.inf))
    return p


@pytest.mark.parametrize("depth", [3, 8])
@pytest.mark.parametrize("scale,min_point", [(1.0, MIN), (2.5, np.array([-1.25, 0.5, -3.0], np.float32))])
def test_place_and_remove_land_on_the_finest_cells(depth, scale, min_point):
    rng = np.random.default_rng(depth)
    floats, ints = _octree(depth, scale, min_point)
    g = 1 << depth
    for normal in NORMALS:
        for _ in range(8):
            cell = rng.integers(1, g - 1, 3)                  # (an interior cell: both neighbours exist)
            uv = rng.uniform(0.05, 0.95, 2)
            for nudge in (-3, 0, 3):
                hit = _hit(_face_point(cell, normal, depth, scale, min_point, uv, nudge), normal)
                place = host.pick_edit_delta(hit, (floats, ints), 1, 7.0)
                remove = host.pick_edit_delta(hit, (floats, ints), 0, 0.0)
                expect_place = ((cell + np.asarray(normal)) + 0.5) / g
                expect_remove = (cell + 0.5) / g
                assert np.array_equal(place[:3], expect_place.astype(np.float32)), (normal, cell, nudge)
                assert np.array_equal(remove[:3], expect_remove.astype(np.float32)), (normal, cell, nudge)
                assert place[3] == 2.0 and place[4] == 7.0 and remove[3] == 0.0 and remove[4] == 0.0
                assert not place[5:].any() and not remove[5:].any()


def test_scene_form_reads_slots_6_and_7():
    scene = host.Scene.demo()
    floats, ints = scene.blobs[6], scene.blobs[7]
    hit = _hit(_face_point(np.array([500, 400, 600]), (0, 1, 0), int(ints[0]), float(floats[4]), floats[:3], (0.5, 0.5), 0), (0, 1, 0))
    assert np.array_equal(host.pick_edit_delta(hit, scene, 1, 3.0), host.pick_edit_delta(hit, (floats, ints), 1, 3.0))


def test_unusable_hits_are_rejected():
    floats, ints = _octree(3)
    good = _face_point(np.array([2, 2, 2]), (1, 0, 0), 3, 1.0, MIN, (0.5, 0.5), 0)
    for bad in (_hit(good, (1, 0, 0), status=rt.RAY_MISS), _hit(good, (1, 0, 0), status=rt.RAY_ITER_LIMIT),
                _hit(good, (1, 0, 0), fresh=0)):
        for place in (0, 1):
            with pytest.raises(ValueError, match="0x501"):
                host.pick_edit_delta(bad, (floats, ints), place, 1.0)
    # placing in front of a face of the octree's own boundary would leave it (point_inside, octree.rs:165-168)
    for normal in NORMALS:
        n = np.asarray(normal)
        cell = np.where(n > 0, 7, np.where(n < 0, 0, 3))
        edge = _hit(_face_point(cell, normal, 3, 1.0, MIN, (0.5, 0.5), 0), normal)
        with pytest.raises(ValueError, match="outside the octree"):
            host.pick_edit_delta(edge, (floats, ints), 1, 1.0)
        assert np.array_equal(host.pick_edit_delta(edge, (floats, ints), 0, 0.0)[:3], ((cell + 0.5) / 8).astype(np.float32))
    with pytest.raises(ValueError):
        host.pick_edit_delta(_hit(good, (1, 0, 0)), (floats, ints), 2, 1.0)
