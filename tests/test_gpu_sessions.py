"""Editing sessions on ONE long-lived context and ONE bound tree (tests/session_model.py): many calls of different units in a row,
each working on what the call before left — shells, filled solids, moved and mirrored selections, trees with dead cells and a
counter past the tree —, through a cells buffer with deliberately little room that is grown into, overrun (the call fails and
writes nothing), shrunk and compacted.  After EVERY step the buffer must hold the bytes of the builder's tree of the model's voxel
list followed by zeros (after a point-edit batch: the oracle's cells), the counter must be right and tdt_octree_extract must return
the model's list; read-only steps must return the model's arrays and leave buffer and counter alone.  The rendered sessions also
render between the steps, twice each time (the second frame is the cost-ordered replay), against the oracle's frame of the model's
cells: every derived table of the trace path is keyed on the buffer's version, and every step bumps it.  A multi-device context
answers reads from its first member, so the two-member session sees its second replica the way the per-unit suites do: through a
frame, which is sharded over the members.

A failing step prints its session — seed, depth and the steps up to it — in a form session_model.apply / Model.step take again.
tests/test_session_model.py asserts on the CPU what these sessions reach."""
import time

import numpy as np
import pytest

import session_model as sm
import tree_model
from test_gpu_connect import bind_tree
from test_gpu_raycast import _assert_first_hit, _lambertian
from test_gpu_region_edit import expected_bytes
from tdt4230_project_raytracing_amd import host, rt

pytestmark = pytest.mark.gpu
W, H = 64, 48


class Bound:
    """One context with the session's tree bound: slot 0 with the session's capacity, the counter at the tree's cell count, the
    octree uniforms in slots 6 / 7 and a delta buffer in slot 5 for the update program.  scene: inside an rt.Renderer over
    session_model.session_scene (one device, or `devices`); else a bare rt.Context through test_gpu_connect.bind_tree."""

    def __init__(self, s, model, scene=False, devices=None):
        self.s, self.renderer = s, None
        n0 = model.counter
        if scene:
            self.cam = host.camera_reference_pose(W, H, 2, 4)
            self.renderer = rt.Renderer(sm.session_scene(s, model.cells), self.cam, devices=devices)
            self.ctx, self.cells = self.renderer.ctx, self.renderer.vbos[0]
            self.counter = rt.VertexBufferObject(self.ctx, np.array([n0], np.uint32))
            self.ctx.bind_buffer_base(rt.ATOMIC_COUNTER_BUFFER, 0, self.counter)
        else:
            self.ctx = rt.Context(0, devices=devices)
            self.cells, self.counter, V = bind_tree(self.ctx, s["V0"], s["depth"], room=s["capacity"] - n0)
            assert np.array_equal(V, model.V) and np.array_equal(s["ints"], [s["depth"], 64, 1 << s["depth"]])
            self.counter.sub_data(0, np.array([n0], np.uint32))        # (bind_tree leaves a marker there; the update program allocates from it)
            self.floats = rt.VertexBufferObject(self.ctx, s["floats"])
            self.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 6, self.floats)
        self.nbytes = 64 * s["capacity"]
        self.delta = rt.VertexBufferObject(self.ctx, np.zeros(8 * 16, np.float32))
        self.ctx.bind_buffer_base(rt.SHADER_STORAGE_BUFFER, 5, self.delta)
        self.update = rt.ComputeShader(self.ctx, rt.PROGRAM_OCTREE_UPDATE)

    def state(self):
        return self.cells.read(np.uint32), int(self.counter.read(np.uint32)[0])

    def close(self):
        (self.renderer or self.ctx).close()


def run_edit(b, step):
    """The call of an edit step; returns the cell count it reports (None for the update program, which reports none)."""
    kind, a = step
    ctx, R = b.ctx, sm.regions_of
    if kind == "region":
        return ctx.octree_edit_region(a["op"], R(a["regions"]), a["material"])
    if kind == "voxels":
        return ctx.octree_edit_voxels(a["op"], a["raw"])
    if kind == "connected":
        return ctx.octree_edit_connected(a["op"], seeds=a["seeds"], regions=R(a["regions"]), connectivity=a["connectivity"], match=a["match"],
                                         min_voxels=a["min_voxels"], max_voxels=a["max_voxels"], invert=a["invert"], material=a["material"])
    if kind == "morph":
        return ctx.octree_morph(a["op"], a["radius"], a["connectivity"], a["material"], a["border"], R(a["regions"]))
    if kind == "round":
        return ctx.octree_morph_round(a["op"], a["radius2"], a["material"], a["border"], R(a["regions"]))
    if kind == "fill":
        return ctx.octree_fill_enclosed(a["connectivity"], a["material"], R(a["regions"]))
    if kind == "triangles":
        return ctx.octree_edit_triangles(a["op"], a["vertices"], a["triangles"], a["materials"], a["material"])
    if kind == "triangles_solid":
        return ctx.octree_edit_triangles_solid(a["op"], a["vertices"], a["triangles"], None, a["material"], a["connectivity"], a["fill_material"])
    if kind == "transform":
        return ctx.octree_transform({k: a[k] for k in ("a", "t", "material", "dst_lo", "dst_hi")}, a["op"], R(a["regions"]))
    if kind == "geodesic":
        return ctx.octree_edit_geodesic(a["op"], a["seeds"], medium=a["medium"], steps=a["steps"], max_cost=a["max_cost"], match=a["match"],
                                        material=a["material"], regions=R(a["regions"]))
    if kind == "points":
        d = np.ascontiguousarray(a["delta"], np.float32).reshape(-1, 8)
        b.delta.sub_data(0, d)
        b.update.dispatch_compute(len(d), 1, 1)
        return None
    if kind == "compact":
        return ctx.octree_compact()
    raise ValueError(kind)


def run_read(b, step):
    kind, a = step
    ctx, R = b.ctx, sm.regions_of
    if kind == "extract":
        return (ctx.octree_extract(),)
    if kind == "extract_region":
        return (ctx.octree_extract_region(R(a["regions"])),)
    if kind == "components":
        return ctx.octree_components(a["connectivity"], a["match"])
    if kind == "surface":
        return (ctx.octree_extract_surface(a["merge"], a["by_material"], R(a["regions"])),)
    if kind == "distance_field":
        return ctx.octree_distance_field(a["lo"], a["hi"], a["max_d2"], a["border"], nearest=True)
    if kind == "geodesic_field":
        return (ctx.octree_geodesic_field(a["seeds"], a["lo"], a["hi"], medium=a["medium"], steps=a["steps"], max_cost=a["max_cost"], match=a["match"],
                                          regions=R(a["regions"])),)
    if kind == "extract_morph":
        return (ctx.octree_extract_morph(a["op"], a["radius"], a["connectivity"], a["material"], a["border"], R(a["regions"])),)
    raise ValueError(kind)


def _same_array(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.size == want.size and (got.size == 0 or (got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()))


def check_step(b, model, i):
    """Step i of the session on the GPU and in the model, and every check that follows a step.  Returns the model's outcome."""
    s = b.s
    step = s["steps"][i]
    kind = step[0]

    def where(what):
        return f"{what} at step {i} ({kind}) of\n{sm.format_session(s, upto=i)}"

    before_cells, before_counter = model.cells, model.counter
    o = model.step(step)
    if o.status == "read":
        got = run_read(b, step)
        assert len(got) == len(o.read), where("the number of arrays")
        for k, (g, w) in enumerate(zip(got, o.read)):
            assert _same_array(g, w), where(f"array {k} of the read")
        cells, counter = b.state()
        assert np.array_equal(cells, before_cells) and counter == before_counter, where("a read-only call changed the buffer or the counter")
        return o
    if o.status == "misfit":
        with pytest.raises(rt.TdtError) as e:
            run_edit(b, step)
        assert e.value.code == rt.ERR_INVALID_VALUE and getattr(e.value, "n_cells", o.n_cells) == o.n_cells, where(f"the misfit error ({e.value})")
        cells, counter = b.state()
        assert np.array_equal(cells, before_cells) and counter == before_counter, where("a misfit wrote something")
    else:
        n = run_edit(b, step)
        if kind == "points":                                          # not canonical: the oracle's cells and counter
            want = o.cells
        else:
            assert n == o.n_cells, where(f"the returned cell count {n}, expected {o.n_cells},")
            want, n_want = expected_bytes(b.ctx, o.V, s["depth"], b.nbytes)          # the GPU builder's tree, pinned to tree_model's
            assert n_want == o.n_cells and np.array_equal(want, o.cells), where("the builder's tree against the model's")
        cells, counter = b.state()
        assert np.array_equal(cells, want), where(f"the cells buffer ({int((cells != want).sum())} words differ)")
        assert counter == o.counter, where(f"the counter {counter}, expected {o.counter},")
    got = b.ctx.octree_extract()
    assert _same_array(got, o.V), where("octree_extract")
    return o


def run_session(name, oracle, after=None, **bound):
    s = sm.session(name, oracle)
    model = sm.model_of(s, oracle)
    b = Bound(s, model, **bound)
    t0 = time.perf_counter()
    try:
        statuses = []
        if after:
            after(b, model, -1, None)
        for i in range(len(s["steps"])):
            o = check_step(b, model, i)
            statuses.append(o.status)
            if after:
                after(b, model, i, o)
        print(f"{name}: {len(s['steps'])} steps in {time.perf_counter() - t0:.2f} s: {' '.join(statuses)}")
        return s, statuses
    finally:
        b.close()


# ---- the editing sessions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sm.EDIT_SESSIONS)
def test_single_device_session(oracle, name):
    """Three sessions of 24 steps at depths 4, 5 and 5 that hold every kind between them, and one of 10 steps over a sparse depth-6
    tree across the word and tile boundaries of the bit-volume layout (the kinds whose models stay fast there)."""
    s, statuses = run_session(name, oracle)
    assert "read" in statuses and statuses.count("ok") >= len(statuses) // 2           # (what the sessions reach: tests/test_session_model.py)


def _model_scene(b, model):
    """tree_model.scene_from_cells around the model's cells: config 1's tables and octree placement, written out independently of the
    scene the renderer was given."""
    like = host.Scene.config(1)
    scene = tree_model.scene_from_cells(model.cells, b.s["depth"], b.s["cell_count"], like)
    assert np.array_equal(scene.blobs[6], b.s["floats"]) and np.array_equal(scene.blobs[7], b.s["ints"])
    return scene


def _frame_is_the_oracles(b, model, oracle, what):
    img = b.renderer.render()
    ref = oracle.render(_model_scene(b, model), b.cam, threads=4)
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
    assert bad == 0, f"{what}: {bad} of {W * H} pixels differ from the oracle's frame of the model's cells"
    return img


def test_two_member_session(oracle):
    """devices = [0, 0]: after every step the first member's cells and counter are read as above, and a frame — sharded over both
    members, so half of it is traced through the second replica's cells — must be the oracle's frame of the model's cells."""
    def after(b, model, i, o):
        assert b.ctx.device_count() == 2
        _frame_is_the_oracles(b, model, oracle, f"the two-member frame after step {i} of\n{sm.format_session(b.s, upto=max(i, 0))}")

    run_session("two_members", oracle, after=after, scene=True, devices=[0, 0])


@pytest.mark.parametrize("name", ["rendered", "rendered_d5"])
def test_rendered_session(oracle, name):
    """An rt.Renderer over host.Scene.config(1) with spare cells appended ("rendered"; "rendered_d5": over a depth-5 tree inside
    that scene's tables): a frame before the first step and after every second one, twice each time, bit for bit the oracle's frame
    of tree_model.scene_from_cells of the model's cells; between two of the renders a pick of all pixels against
    the oracle's first hits.  The depth-3 scene has one specialised build, so its variant must stay; at depth 5 the whole-depth
    table serves the tree exactly while session_model.whole_depth_table_fits says so, which a point-edit batch ends and a later
    rebuild restores: last_variant() must follow the model and change over the session."""
    variants, picked = [], []
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.int32)

    def after(b, model, i, o):
        if i >= 0 and i % 2 == 0:
            return
        what = f"after step {i} of\n{sm.format_session(b.s, upto=max(i, 0))}"
        if i == -1 and name == "rendered":                            # the scene is config 1's own, with spare cells
            like = host.Scene.config(1)
            scene = sm.session_scene(b.s, model.cells)
            assert all(np.array_equal(scene.blobs[k], like.blobs[k]) for k in (1, 2, 3, 4, 6, 7))
            own = np.ascontiguousarray(like.blobs[0]).view(np.uint32)
            assert np.array_equal(model.cells[: len(own)], own) and not model.cells[len(own):].any() and len(model.cells) > len(own)
        first = _frame_is_the_oracles(b, model, oracle, "the frame " + what)
        v = b.ctx.last_variant()
        again = _frame_is_the_oracles(b, model, oracle, "the cost-ordered replay " + what)
        assert again.tobytes() == first.tobytes() and b.ctx.last_variant() == v
        assert v["depth"] == b.s["depth"] and v["resident"] == 1, (v, what)
        if b.s["depth"] in (5, 6):
            assert v["full"] == int(sm.whole_depth_table_fits(model.cells, b.s["depth"])), (v, what)
        variants.append(tuple(sorted(v.items())))
        if i == 3:                                                    # between two renders: what is under every pixel
            hits, rays = b.renderer.pick(xy, sample=1, return_rays=True)
            assert b.ctx.raycast(rays).tobytes() == hits.tobytes()
            lamb, alb = _lambertian(_model_scene(b, model))
            cam1 = b.cam.copy()
            cam1.max_bounce = 1
            picked.append(_assert_first_hit(oracle, lamb, alb, cam1, hits, rays, 1, W, H))

    s, statuses = run_session(name, oracle, after=after, scene=True)
    kinds = [k for k, _ in s["steps"]]
    assert "points" in kinds and "compact" in kinds
    assert len(variants) == 6 and picked and picked[0][0] > 0
    if name == "rendered":
        assert len(set(variants)) == 1
    else:
        assert len(set(variants)) > 1, variants
