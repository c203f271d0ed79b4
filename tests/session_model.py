"""Editing sessions as data, and their model.  A session is what a user of ONE long-lived context does: one bound tree, many
calls of different units in a row, each working on what the call before left.  A step is a plain tuple (kind, args) of ints,
floats and small lists / arrays, so that a failing session can be printed (format_session) and replayed by hand:

    V = sort_vox(session["V0"])
    for step in session["steps"]:
        V = apply(V, session["depth"], step)

apply() only dispatches to the models the per-unit suites already use (test_gpu_region_edit.apply_op / expected_region,
connect_model, morph_model, distance_model, fill_model, mesh_model, xform_model, geodesic_model); it restates none of them.  The two
kinds that are no function of V alone — a batch of point edits through the update program, which is expected through the oracle's
restatement of that program, and the compaction that follows it — go through Model, which carries the cells buffer and the counter
next to V and marks the steps whose canonical tree does not fit the buffer ("misfit": the call fails and nothing is written).

generate() draws a session from a seed.  It runs the model while it draws, so that brushes are aimed at what the tree holds at that
step.  SESSION_SPECS lists the committed sessions; tests/test_session_model.py asserts on the CPU that they are worth running and
tests/test_gpu_sessions.py runs them on the GPU."""
import numpy as np

import connect_model
import distance_model
import fill_model
import geodesic_model
import mesh_model
import morph_model
import oracle_py
import surface_model
import tree_model
import xform_model
from octree_util import distinct_deltas, expand_cells
from test_gpu_region_edit import apply_op, expected_region, inside, morton, sort_vox
from tdt4230_project_raytracing_amd import host, rt

EDIT_KINDS = ("region", "voxels", "connected", "morph", "round", "fill", "triangles", "triangles_solid", "transform", "geodesic",
              "points", "compact")
READ_KINDS = ("extract", "extract_region", "components", "surface", "distance_field", "geodesic_field", "extract_morph")
ALL_KINDS = EDIT_KINDS + READ_KINDS
# the kinds whose models stay fast on a 64^3 grid (the distance transform and the bucket relaxation take seconds there)
FAST_KINDS = tuple(k for k in ALL_KINDS if k not in ("round", "distance_field", "geodesic", "geodesic_field"))
REFILL_KINDS = ("region", "voxels", "triangles", "triangles_solid")        # what can put voxels into an empty tree


# ---- steps as data ---------------------------------------------------------------------------------------------------------
def regions_of(spec):
    """None, or a list of ("box", lo, hi) / ("sphere", centre, radius) -> None, or the rt.Region list."""
    if spec is None:
        return None
    return [rt.box(g[1], g[2]) if g[0] == "box" else rt.sphere(g[1], g[2]) for g in spec]


def xform_of(a):
    return xform_model.X(a["a"], a["t"], a["material"], a["dst_lo"], a["dst_hi"])


def list_meaning(raw, depth):
    """What tdt_octree_edit_voxels makes of a raw list: entries off the grid dropped, the last of a position's entries wins."""
    n = 1 << depth
    last = {}
    for v in np.asarray(raw, np.int64).reshape(-1, 4):
        if (v[:3] >= 0).all() and (v[:3] < n).all():
            last[tuple(int(c) for c in v[:3])] = int(v[3])
    return np.array([[*k, m] for k, m in last.items()], np.int32).reshape(-1, 4)


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    if isinstance(v, (list, tuple)):
        return type(v)(_plain(e) for e in v)
    if isinstance(v, dict):
        return {k: _plain(e) for k, e in v.items()}
    return v


def format_session(session, upto=None):
    """The session up to and including step `upto` as python text that evaluates to what apply() / Model.step() take again."""
    steps = session["steps"] if upto is None else session["steps"][: upto + 1]
    head = {k: _plain(session[k]) for k in ("name", "seed", "depth", "capacity", "cell_count") if k in session}
    lines = [f"session {head}", f"V0 = {_plain(np.asarray(session['V0']))}", "steps = ["]
    lines += [f"    {(_plain(k), _plain(a))!r}," for k, a in steps]
    return "\n".join(lines + ["]"])


# ---- the model of the steps that are functions of V ------------------------------------------------------------------------------
def _brush(V, depth, kind, a):
    """The voxel list B of the kinds that are octree_edit_voxels(op, B)."""
    if kind == "voxels":
        return list_meaning(a["raw"], depth)
    if kind == "triangles":
        return mesh_model.voxelize(a["vertices"], a["triangles"], depth, a["materials"], a["material"])
    if kind == "triangles_solid":
        surface = mesh_model.voxelize(a["vertices"], a["triangles"], depth, None, a["material"])
        return fill_model.filled(surface, depth, a["connectivity"], a["fill_material"])
    if kind == "transform":
        return xform_model.transform(V, depth, xform_of(a), regions_of(a["regions"]))
    if kind == "geodesic":
        return geodesic_model.reach_list(V, depth, np.asarray(a["seeds"]).reshape(-1, 3), material=a["material"], medium=a["medium"],
                                         steps=tuple(a["steps"]), max_cost=a["max_cost"], match=a["match"], regions=regions_of(a["regions"]))
    raise ValueError(kind)


def apply(V, depth, step):
    """The Morton-sorted voxel list after `step` on the tree of V.  Read-only kinds and compact leave V; a point-edit batch is no
    function of V (Model.step)."""
    kind, a = step
    V = sort_vox(V)
    if kind in READ_KINDS or kind == "compact":
        return V
    if kind == "region":
        return expected_region(V, a["op"], regions_of(a["regions"]), a["material"], depth)
    if kind in ("voxels", "triangles", "triangles_solid", "transform", "geodesic"):
        return apply_op(V, a["op"], _brush(V, depth, kind, a), 0)
    if kind == "connected":
        return connect_model.edit(V, depth, a["op"], a["material"], a["connectivity"], a["match"], seeds=a["seeds"], regions=regions_of(a["regions"]),
                                  min_voxels=a["min_voxels"], max_voxels=a["max_voxels"], invert=a["invert"])
    if kind == "morph":
        return morph_model.morph(V, depth, a["op"], a["radius"], a["connectivity"], a["material"], a["border"], regions_of(a["regions"]))
    if kind == "round":
        return distance_model.round_op(V, depth, a["op"], a["radius2"], a["material"], a["border"], regions_of(a["regions"]))
    if kind == "fill":
        return fill_model.filled(V, depth, a["connectivity"], a["material"], regions_of(a["regions"]))
    if kind == "points":
        raise ValueError("a point-edit batch acts on the cells, not on V: run it through Model.step")
    raise ValueError(kind)


def observe(V, depth, step):
    """What a read-only step returns on the tree of V, as a tuple of arrays."""
    kind, a = step
    V = sort_vox(V)
    if kind == "extract":
        return (V,)
    if kind == "extract_region":
        return (V[inside(V[:, :3], regions_of(a["regions"]))],)
    if kind == "components":
        labels, tab = connect_model.components(V, depth, a["connectivity"], a["match"])
        return labels, tab
    if kind == "surface":
        return (np.asarray(surface_model.quads(V, depth, a["merge"], a["by_material"], regions_of(a["regions"])), np.int32).reshape(-1, 8),)
    if kind == "distance_field":
        return distance_model.field(V, depth, a["lo"], a["hi"], a["max_d2"], a["border"])
    if kind == "geodesic_field":
        return (geodesic_model.field(V, depth, np.asarray(a["seeds"]).reshape(-1, 3), a["lo"], a["hi"], medium=a["medium"], steps=tuple(a["steps"]),
                                     max_cost=a["max_cost"], match=a["match"], regions=regions_of(a["regions"])),)
    if kind == "extract_morph":
        return (morph_model.morph(V, depth, a["op"], a["radius"], a["connectivity"], a["material"], a["border"], regions_of(a["regions"])),)
    raise ValueError(kind)


# ---- the model of the buffer ---------------------------------------------------------------------------------------------------
def canonical_cells(V, depth):
    """The builder's tree of V as uint32 words: tree_model's, which the GPU suites pin the GPU builder to."""
    return tree_model.build_cells(V, depth) if len(V) else np.zeros(16, np.uint32)


def walk(cells, depth):
    """The voxels a walk of `cells` reaches, Morton-sorted (tests/test_gpu_octree_compact.py's numpy walk)."""
    return sort_vox(expand_cells(cells, depth))


def octree_uniforms(depth, cell_count):
    """(OctreeFloats, OctreeInts) of a unit-cube octree at the origin: what slots 6 and 7 hold for the update program.  cell_count is
    a power of two, so that the program's float index arithmetic ((value + f) / cell_count * 2 cell_count) is exact."""
    assert cell_count & (cell_count - 1) == 0
    floats = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, np.float32(1.0) / np.float32(cell_count)], np.float32)
    return floats, np.array([depth, 64, cell_count], np.int32)


class Outcome:
    """What a step must leave: status "ok" / "noop" (an edit that changed neither V nor, for compact, the cell count) / "misfit" /
    "read"; the model's V, cells (capacity cells, uint32) and counter after it; n_cells, the count an edit call returns or, for a
    misfit, the count its error reports; read: the arrays a read-only step returns."""

    def __init__(self, status, model, n_cells=None, read=None):
        self.status, self.n_cells, self.read = status, n_cells, read
        self.V, self.cells, self.counter, self.canonical = model.V, model.cells, model.counter, model.canonical


class Model:
    """V, the cells buffer of `capacity` cells and the counter of one session.  floats / ints: the slot 6 / 7 payloads the update
    program reads (octree_uniforms, or a scene's)."""

    def __init__(self, V0, depth, capacity, floats=None, ints=None, oracle=None):
        self.depth, self.capacity, self.oracle = depth, capacity, oracle
        self.floats, self.ints = (floats, ints) if floats is not None else octree_uniforms(depth, 1 << depth)
        self.V = sort_vox(V0)
        built = canonical_cells(self.V, depth)
        assert len(built) // 16 <= capacity
        self._install(built)

    def _install(self, built):
        self.cells = np.zeros(16 * self.capacity, np.uint32)
        self.cells[: len(built)] = built
        self.counter = len(built) // 16
        self.canonical = True

    def used_cells(self):
        """Cells the tree occupies: the canonical count, or after point edits what the counter has handed out."""
        return self.counter

    def step(self, step):
        kind, a = step
        if kind in READ_KINDS:
            return Outcome("read", self, read=observe(self.V, self.depth, step))
        if kind == "points":
            scene = host.Scene({0: self.cells, 6: self.floats, 7: self.ints})
            delta = np.ascontiguousarray(a["delta"], np.float32).reshape(-1, 8)
            cells, counter = oracle_py.oracle_octree_update(self.oracle, scene, delta, self.counter, (len(delta), 1, 1))
            assert counter <= self.capacity, "a point-edit batch that outgrows the buffer is not a step the sessions draw"
            before = self.V
            self.cells, self.counter, self.canonical = np.ascontiguousarray(cells).view(np.uint32).reshape(-1), counter, False
            self.V = walk(self.cells, self.depth)
            return Outcome("noop" if np.array_equal(self.V, before) else "ok", self, n_cells=counter)
        V2 = apply(self.V, self.depth, step)
        built = canonical_cells(V2, self.depth)
        need = len(built) // 16
        if need > self.capacity:
            return Outcome("misfit", self, n_cells=need)
        same = np.array_equal(V2, self.V) and (kind != "compact" or need >= self.counter)
        self.V = V2
        self._install(built)
        return Outcome("noop" if same else "ok", self, n_cells=need)


# ---- drawing a session ---------------------------------------------------------------------------------------------------------
def _shell(lo, hi, m):
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    wall = ((g == np.asarray(lo)) | (g == np.asarray(hi))).any(1)
    return np.concatenate([g[wall], np.full((int(wall.sum()), 1), m)], 1).astype(np.int32)


def _block(lo, hi, m):
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([g, np.full((len(g), 1), m)], 1).astype(np.int32)


def initial_tree(rng, depth, materials, sparse=False):
    """A hollow box of one material whose cavity holds aligned 2^3 blocks (filling it merges them), a solid aligned block (a LEAF
    above the finest level from the start), a two-voxel speck and scattered voxels.  sparse (depth 6): the box spans 27 .. 37 on
    every axis, across the 32-voxel word boundary and an 8 x 8 tile boundary of the bit-volume layout, and little else."""
    n = 1 << depth
    m = lambda: int(rng.integers(1, materials + 1))  # noqa: E731
    if sparse:
        parts = [_shell((27, 27, 27), (37, 37, 37), m()), _block((40, 24, 30), (43, 27, 33), m())]
        scattered = rng.integers(22, 44, (40, 3))
    else:
        lo = 2 * rng.integers(0, n // 4 - 1, 3) + 1
        parts = [_shell(lo, lo + 7, m()), _block((n - 4, n - 4, 0), (n - 1, n - 1, 3), m()), _block((0, n - 2, n - 1), (1, n - 2, n - 1), m())]
        scattered = rng.integers(0, n, (n * 3, 3))
    parts.append(np.concatenate([scattered, rng.integers(1, materials + 1, (len(scattered), 1))], 1).astype(np.int32))
    V = np.concatenate(parts)
    _, first = np.unique(morton(V[:, :3]), return_index=True)             # (the first part listed at a position keeps it)
    return sort_vox(V[np.sort(first)])


class _Draw:
    """The draws of one session: every method returns the args of one step, aimed at the model's current V."""

    def __init__(self, rng, depth, materials, model):
        self.rng, self.depth, self.n, self.materials, self.model = rng, depth, 1 << depth, materials, model

    def mat(self):
        return int(self.rng.integers(0, self.materials))

    def mat_or_none(self):
        return None if self.rng.random() < 0.5 else self.mat()

    def voxel(self):
        V = self.model.V
        return V[int(self.rng.integers(len(V))), :3].astype(int) if len(V) else np.full(3, self.n // 2)

    def centre(self):
        """An occupied voxel, or (one time in three) a point pushed to a face of the grid, so that the shape hangs over it."""
        c = self.voxel()
        if self.rng.random() < 0.33:
            c[int(self.rng.integers(3))] = int(self.rng.choice([0, self.n - 1]))
        return c

    def shape(self, big=1):
        c, r = self.centre(), int(self.rng.integers(1, 2 + big * max(1, self.n // 8)))
        if self.rng.random() < 0.5:
            return ("sphere", c.tolist(), r)
        e = self.rng.integers(0, r + 1, 3)
        return ("box", (c - e).tolist(), (c + self.rng.integers(0, r + 1, 3)).tolist())

    def regions(self, big=1):
        return [self.shape(big)] + ([self.shape(big)] if self.rng.random() < 0.33 else [])

    def mask(self, p=0.4):
        return self.regions(2) if self.rng.random() < p else None

    def field_box(self):
        c = self.voxel()
        lo = np.clip(c - self.rng.integers(1, self.n // 4 + 1, 3), 0, self.n - 1)
        hi = np.clip(c + self.rng.integers(1, self.n // 4 + 1, 3), 0, self.n - 1)
        return lo.tolist(), hi.tolist()

    # -- edits --
    def region(self):
        if self.rng.random() < 0.1 and len(self.model.V):                 # the whole grid, and past it: through the empty tree
            return dict(op=rt.REGION_CLEAR, regions=[("box", [-2, -1, 0], [self.n + 1, self.n, self.n - 1])], material=0)
        return dict(op=int(self.rng.integers(4)), regions=self.regions(), material=self.mat())

    def voxels(self):
        """In the manner of test_gpu_voxlist.raw_list: voxels of V and fresh ones, some listed again later with another material
        (the later one wins), and one entry off the grid."""
        V, k = self.model.V, int(self.rng.integers(16, 48))
        pts = self.rng.integers(0, self.n, (k, 3))
        if len(V):
            pts[: k // 2] = V[self.rng.integers(0, len(V), k // 2), :3]
        lst = np.concatenate([pts, self.rng.integers(1, self.materials + 1, (k, 1))], 1)
        dup = lst[2:8].copy()
        dup[:, 3] = dup[:, 3] % self.materials + 1
        off = [[self.n, 3, 3, 1]] if self.rng.random() < 0.5 else [[2, -1, 5, 1]]
        raw = np.concatenate([lst[: k // 2], off, lst[k // 2:], dup]).astype(np.int32)
        return dict(op=int(self.rng.choice([rt.REGION_SET, rt.REGION_FILL])), raw=raw)

    def connected(self):
        a = dict(op=int(self.rng.choice([rt.REGION_PAINT, rt.REGION_CLEAR])), seeds=None, regions=None, connectivity=int(self.rng.choice([6, 26])),
                 match=int(self.rng.choice([rt.MATCH_ANY, rt.MATCH_MATERIAL])), min_voxels=0, max_voxels=2 ** 32 - 1, invert=False, material=self.mat())
        form = int(self.rng.integers(3))
        if form == 0:
            a["seeds"] = [self.voxel().tolist(), [-1, 2, 3]]
            a["invert"] = bool(self.rng.random() < 0.15)
        elif form == 1:
            a["regions"] = [self.shape()]
        elif self.rng.random() < 0.5:
            a["max_voxels"] = int(self.rng.integers(1, 4))                # the specks
        else:
            a["min_voxels"], a["match"] = int(self.rng.integers(8, 40)), rt.MATCH_ANY
        return a

    def morph(self):
        """(The library's morphology knows the 6- and the 26-neighbourhood; there is no 18.)"""
        op = int(self.rng.integers(5))
        radius = int(self.rng.integers(1, 3))
        conn = int(self.rng.choice([6, 26]))
        if op == rt.MORPH_DILATE and radius == 2:                         # (two steps of 26 neighbours fill most of a small grid)
            conn = 6
        return dict(op=op, radius=radius, connectivity=conn, material=self.mat_or_none(), border=int(self.rng.integers(2)), regions=self.mask())

    def round(self):
        return dict(op=int(self.rng.integers(5)), radius2=int(self.rng.choice([1, 2, 3, 4, 5, 6, 8, 9])), material=self.mat_or_none(),
                    border=int(self.rng.integers(2)), regions=self.mask())

    def fill(self):
        return dict(connectivity=int(self.rng.choice([6, 26])), material=self.mat_or_none(), regions=self.mask(0.2))

    def _sphere_mesh(self):
        c = self.voxel() + self.rng.random(3)
        v, t = mesh_model.uv_sphere(c, float(self.rng.uniform(1.6, max(2.0, self.n / 6))), 5, 6)
        return mesh_model.quantize(v).astype(np.int32), t

    def triangles(self):
        if self.rng.random() < 0.5:
            v, t = self._sphere_mesh()
        else:
            v, t, _ = mesh_model.random_triangles(self.rng, int(self.rng.integers(3, 7)), self.n, kinds=("general", "lattice", "segment", "point", "plane"))
            far = np.abs(v.astype(np.int64).reshape(-1, 3, 3) - v.astype(np.int64).reshape(-1, 3, 3)[:, :1]).max((1, 2)) > 6 * mesh_model.UNIT
            keep = ~far                                                   # (a triangle across the whole grid would outgrow every buffer)
            if not keep.any():
                keep[0] = True
            v = v.reshape(-1, 3, 3)[keep].reshape(-1, 3)
            t = np.arange(len(v), dtype=np.uint32).reshape(-1, 3)
        mats = self.rng.integers(1, self.materials + 1, len(t)).astype(np.int32) if self.rng.random() < 0.5 else None
        return dict(op=int(self.rng.integers(4)), vertices=v, triangles=t, materials=mats, material=self.mat())

    def triangles_solid(self):
        v, t = self._sphere_mesh()
        return dict(op=int(self.rng.choice([rt.REGION_SET, rt.REGION_FILL, rt.REGION_CLEAR])), vertices=v, triangles=t, material=self.mat(),
                    connectivity=int(self.rng.choice([6, 26])), fill_material=self.mat_or_none())

    def transform(self):
        n, c = self.n, self.voxel()
        pivot2 = [n, n, n] if self.rng.random() < 0.5 else (2 * c + 1).tolist()
        form = int(self.rng.integers(5))
        regions = self.mask()
        if form == 0:
            x = xform_model.translate(self.rng.integers(-3, 4, 3).tolist())
        elif form == 1:
            x = xform_model.quarter_turns(int(self.rng.integers(3)), int(self.rng.integers(1, 4)), pivot2)
        elif form == 2:
            x = xform_model.mirror(int(self.rng.integers(3)), pivot2)
        elif form == 3:
            x = xform_model.scale((1, 1, 1), (2, 2, 2), pivot2)
        else:
            x = xform_model.scale((2, 2, 2), (1, 1, 1), (2 * c + 1).tolist())
            regions = [("sphere", c.tolist(), 2)]                         # (the whole tree doubled would outgrow every buffer)
        f = x.with_(material=self.mat_or_none()).fields()
        return dict(op=int(self.rng.choice([rt.REGION_SET, rt.REGION_FILL])), a=f["a"], t=f["t"], material=f["material"], dst_lo=f["dst_lo"],
                    dst_hi=f["dst_hi"], regions=regions)

    def _steps(self):
        return list([rt.STEPS_6, rt.STEPS_26, rt.CHAMFER_345][int(self.rng.integers(3))])

    def geodesic(self):
        steps = self._steps()
        if self.rng.random() < 0.3:                                       # pour a little material into the air next to a voxel
            seed = np.clip(self.voxel() + self.rng.integers(-1, 2, 3), 0, self.n - 1)
            return dict(op=rt.REGION_FILL, seeds=[seed.tolist()], medium=rt.MEDIUM_EMPTY, steps=steps, max_cost=int(steps[0] * self.rng.integers(1, 3)),
                        match=None, material=self.mat(), regions=None)
        op = int(self.rng.choice([rt.REGION_PAINT, rt.REGION_CLEAR, rt.REGION_SET]))
        return dict(op=op, seeds=[self.voxel().tolist(), self.voxel().tolist()], medium=rt.MEDIUM_SOLID, steps=steps,
                    max_cost=int(steps[0] * self.rng.integers(1, 8)), match=None, material=None if op == rt.REGION_CLEAR else self.mat(), regions=self.mask(0.2))

    def points(self):
        """Places and removes, each in its own cell of the level the update program's walk ends on and no two writing one node; as
        many as the buffer has cells for (the model runs the batch to see)."""
        m = self.model
        count = int(self.rng.integers(4, 10))
        d = distinct_deltas(self.rng, count, self.depth, m.cells)
        d[:, 3] = np.where(np.arange(len(d)) % 3 == 2, 0.0, 2.0)          # two places, one remove, ..
        d[:, 4] = np.where(d[:, 3] == 2.0, self.rng.integers(0, self.materials, len(d)), 0)
        scene = host.Scene({0: m.cells, 6: m.floats, 7: m.ints})
        while len(d):
            _, counter = oracle_py.oracle_octree_update(m.oracle, scene, d, m.counter, (len(d), 1, 1))
            if counter <= m.capacity:
                return dict(delta=np.ascontiguousarray(d, np.float32))
            d = d[: len(d) // 2]
        return None

    def compact(self):
        return {}

    # -- reads --
    def extract(self):
        return {}

    def extract_region(self):
        return dict(regions=self.regions(2))

    def components(self):
        return dict(connectivity=int(self.rng.choice([6, 26])), match=int(self.rng.choice([rt.MATCH_ANY, rt.MATCH_MATERIAL])))

    def surface(self):
        return dict(merge=int(self.rng.integers(2)), by_material=int(self.rng.integers(2)), regions=self.mask())

    def distance_field(self):
        lo, hi = self.field_box()
        return dict(lo=lo, hi=hi, max_d2=int(self.rng.choice([1, 4, 9, 30, 64])), border=int(self.rng.integers(2)))

    def geodesic_field(self):
        lo, hi = self.field_box()
        medium = rt.MEDIUM_SOLID if self.rng.random() < 0.7 else rt.MEDIUM_EMPTY
        seed = self.voxel() if medium == rt.MEDIUM_SOLID else np.clip(self.voxel() + [0, 1, 0], 0, self.n - 1)
        steps = self._steps()
        return dict(seeds=[seed.tolist()], lo=lo, hi=hi, medium=medium, steps=steps, max_cost=int(steps[0] * self.rng.integers(2, 12)), match=None,
                    regions=None)

    def extract_morph(self):
        return self.morph()


def generate(seed, depth, n_steps, kinds, materials=254, room=32, sparse=False, cell_count=None, floats=None, ints=None, oracle=None, name=None, V0=None):
    """Draw a session: {"name", "seed", "depth", "capacity", "cell_count", "V0", "steps"}.  The kinds come in shuffled rounds of
    `kinds`, so that a session of len(kinds) steps holds every one; a compact is drawn behind a point-edit batch, and an empty tree
    is followed by a kind that can fill it.  capacity: the cells of V0's tree plus `room` — deliberately little, so that some
    growing steps do not fit.  V0: the tree to start from instead of initial_tree's.  floats / ints: the slot 6 / 7 payloads of a scene the session runs inside (default: octree_uniforms)."""
    rng = np.random.default_rng(seed)
    V0 = initial_tree(rng, depth, materials, sparse) if V0 is None else sort_vox(V0)
    capacity = len(canonical_cells(V0, depth)) // 16 + room
    if floats is None:
        floats, ints = octree_uniforms(depth, cell_count or (1 << depth))
    model = Model(V0, depth, capacity, floats, ints, oracle)
    draw = _Draw(rng, depth, materials, model)
    order = []
    while len(order) < 2 * n_steps:
        order += [kinds[i] for i in rng.permutation(len(kinds))]
    steps = []
    while len(steps) < n_steps:
        kind = order.pop(0)
        if not len(model.V) and kind not in REFILL_KINDS + ("extract", "extract_region"):
            kind = REFILL_KINDS[int(rng.integers(2))]
        if kind == "compact" and model.canonical and "points" in kinds:   # a compact of a canonical tree changes nothing: edit first
            order.insert(int(rng.integers(0, 2)), "compact")
            kind = "points"
        args = getattr(draw, kind)()
        if args is None:                                                  # (no room for a point edit)
            continue
        steps.append((kind, args))
        model.step(steps[-1])
    return {"name": name or f"seed{seed}_d{depth}", "seed": seed, "depth": depth, "capacity": capacity, "cell_count": int(ints[2]), "V0": V0,
            "floats": floats, "ints": ints, "steps": steps}


def model_of(session, oracle=None):
    return Model(session["V0"], session["depth"], session["capacity"], session["floats"], session["ints"], oracle)


# ---- the committed sessions ----------------------------------------------------------------------------------------------------
# the kinds of the two rendered sessions: ten, so that a ten-step session holds a point-edit batch and a compact
RENDER_KINDS = ("region", "voxels", "connected", "morph", "fill", "triangles", "transform", "points", "compact", "extract")
# name: (seed, depth, steps, kinds, options).  The seeds were searched on the CPU for the conditions tests/test_session_model.py
# asserts; nothing else here was.  The sessions with in_scene run inside host.Scene.config(1)'s material table (4 materials) and
# octree uniforms (cell count 128); "rendered" starts from that scene's own tree (depth 3), the others from initial_tree.
SESSION_SPECS = {
    "d4": (6, 4, 24, ALL_KINDS, dict(room=24)),
    "d5a": (0, 5, 24, ALL_KINDS, dict(room=48)),
    "d5b": (23, 5, 24, ALL_KINDS, dict(room=48)),
    "d6": (10, 6, 10, FAST_KINDS, dict(room=64, sparse=True)),
    "two_members": (29, 4, 12, ALL_KINDS, dict(room=24, materials=4, in_scene=True)),
    "rendered": (8, 3, 10, RENDER_KINDS, dict(room=24, materials=4, in_scene=True, config1=True)),
    "rendered_d5": (0, 5, 10, RENDER_KINDS, dict(room=48, materials=4, in_scene=True)),
}
EDIT_SESSIONS = ("d4", "d5a", "d5b", "d6")


def scene_uniforms(depth):
    """The slot 6 / 7 payloads of host.Scene.config(1) with the tree depth replaced: its corner, scale and cell count (128, a power
    of two)."""
    like = host.Scene.config(1)
    ints = np.asarray(like.blobs[7]).view(np.int32).copy()
    ints[0] = depth
    return np.asarray(like.blobs[6]).view(np.float32).copy(), ints


def session(name, oracle=None, seed=None):
    spec_seed, depth, n_steps, kinds, opt = SESSION_SPECS[name]
    opt = dict(opt)
    if opt.pop("in_scene", False):
        opt["floats"], opt["ints"] = scene_uniforms(depth)
    if opt.pop("config1", False):
        like = host.Scene.config(1)
        assert like.max_depth == depth
        opt["V0"] = walk(np.ascontiguousarray(like.blobs[0]).view(np.uint32), depth)
    return generate(spec_seed if seed is None else seed, depth, n_steps, kinds, oracle=oracle, name=name, **opt)


def session_scene(s, cells):
    """The scene a session with in_scene runs in, around `cells`: config 1's material tables and the session's octree uniforms."""
    like = host.Scene.config(1)
    return host.Scene({**{k: like.blobs[k].copy() for k in (1, 2, 3, 4)}, 0: np.ascontiguousarray(cells, np.uint32), 6: s["floats"], 7: s["ints"]},
                      name="session_" + s["name"])


# ---- what a session is worth ---------------------------------------------------------------------------------------------------
def merged_leaves(cells, depth):
    """The number of LEAFs above the finest level (blocks of at least 2^3 voxels) a walk of the tree reaches."""
    c = np.asarray(cells, np.uint32).reshape(-1, 8, 2)
    cell, count = np.zeros(1, np.int64), 0
    for level in range(1, depth):
        nodes = c[cell]
        count += int((nodes[..., 1] == tree_model.LEAF).sum())
        cell = nodes[..., 0][nodes[..., 1] == tree_model.PARENT].astype(np.int64)
        if not cell.size:
            break
    return count


def whole_depth_table_fits(cells, depth):
    """Whether the trace path may serve a depth-5 / 6 tree with its whole-depth table build (last_variant()["full"]): the
    documented claim that table rests on is that a PARENT of level 1 or 2 holds a cell index below 128, one of level 3 an index below
    1024 and a deeper one an index below 8192 (csrc/trace_device.hpp grid_v_bound).  A canonical tree numbers its cells breadth
    first and keeps to it; cells that point edits allocate behind the tree do not."""
    c = np.asarray(cells, np.uint32).reshape(-1, 8, 2)
    cell = np.zeros(1, np.int64)
    for level in range(1, depth):
        nodes = c[cell]
        v = nodes[..., 0][nodes[..., 1] == tree_model.PARENT].astype(np.int64)
        if (v >= (128 if level < 3 else 1024 if level == 3 else 8192)).any():
            return False
        cell = v[v < len(c)]
        if not cell.size:
            break
    return True


def summarise(s, oracle):
    """Run a session through the model alone: {"kinds": count of each kind, "edits", "noops", "misfits", "nonempty" (steps after
    which V holds a voxel), and the steps at which each condition of tests/test_session_model.py is met}."""
    m = model_of(s, oracle)
    out = {"name": s["name"], "steps": len(s["steps"]), "kinds": {}, "edits": 0, "noops": [], "misfits": [], "misfit_then_fit": [], "nonempty": 0,
           "empty": [], "back_from_empty": [], "merging_fill_or_close": [], "edit_on_point_edited_tree": [], "compact_lowers": [], "table_flips": [],
           "status": []}
    fits = whole_depth_table_fits(m.cells, m.depth)
    for i, step in enumerate(s["steps"]):
        kind, a = step
        before_cells, before_counter, before_canonical, before_empty = m.cells, m.counter, m.canonical, len(m.V) == 0
        o = m.step(step)
        out["kinds"][kind] = out["kinds"].get(kind, 0) + 1
        out["status"].append(o.status)
        out["nonempty"] += len(o.V) > 0
        if kind in EDIT_KINDS:
            out["edits"] += 1
            if o.status == "noop":
                out["noops"].append(i)
            if o.status == "misfit":
                out["misfits"].append(i)
            elif out["misfits"] and not out["misfit_then_fit"] and o.status == "ok":
                out["misfit_then_fit"].append(i)
            if len(o.V) == 0 and not before_empty:
                out["empty"].append(i)
            if len(o.V) and before_empty:
                out["back_from_empty"].append(i)
            closing = kind == "fill" or (kind in ("morph", "round") and a["op"] == rt.MORPH_CLOSE)
            if closing and o.status == "ok" and merged_leaves(o.cells, m.depth) > merged_leaves(before_cells, m.depth):
                out["merging_fill_or_close"].append(i)
            if kind not in ("points", "compact") and o.status != "misfit" and not before_canonical and before_counter > len(canonical_cells(walk(before_cells, m.depth), m.depth)) // 16:
                out["edit_on_point_edited_tree"].append(i)
            if kind == "compact" and not before_canonical and o.status == "ok" and o.n_cells < before_counter:
                out["compact_lowers"].append(i)
            now = whole_depth_table_fits(o.cells, m.depth)
            if now != fits:
                out["table_flips"].append(i)
            fits = now
    return out


def summary_text(r):
    kinds = " ".join(f"{k}:{v}" for k, v in sorted(r["kinds"].items()))
    bad = len(r["noops"]) + len(r["misfits"])
    return (f"{r['name']}: {r['steps']} steps, {r['edits']} edits | {kinds} | no-ops {r['noops']} misfits {r['misfits']} = {bad}/{r['edits']} of the edits"
            f" | non-empty after {r['nonempty']}/{r['steps']} | empty at {r['empty']} back at {r['back_from_empty']} | misfit then fit {r['misfit_then_fit']}"
            f" | merging fill/close {r['merging_fill_or_close']} | unit edit on a point-edited tree {r['edit_on_point_edited_tree']}"
            f" | compact lowers {r['compact_lowers']} | whole-depth table flips {r['table_flips']}")
