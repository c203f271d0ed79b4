"""ctypes binding of libtdtrt.so (include/tdt_rt.h) and a Python mirror of the reference's
`src/renderer` wrapper API over it (same names and argument meaning, so tests read like the
reference's host code in main.rs:156-470, 579):

    ComputeShader(ctx).dispatch_compute(w, h, d)      compute_shader.rs:15-38
    Program.set_i32 / set_f32 / set_vector3_f32 / set_vector3_i32     program.rs:35-83
    VertexBufferObject(ctx, array) + bind_buffer_base(SSBO, slot, vbo)  vbo.rs:32-55, main.rs:352
    Texture.new_2d(ctx, w, h)                         texture.rs:47-75

There is no fallback: if the library or a HIP device is missing, construction raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TDT_LIB: alternative build of the same library (A/B experiments); never a different implementation
LIB_PATH = os.environ.get("TDT_LIB") or os.path.join(_HERE, "libtdtrt.so")

OK, ERR_NO_DEVICE, ERR_HIP, ERR_VARIABLE_NOT_FOUND, ERR_INCOMPLETE = 0, 1, 2, 3, 4
ERR_INVALID_ENUM, ERR_INVALID_VALUE, ERR_INVALID_OPERATION = 0x0500, 0x0501, 0x0502
PROGRAM_RAYTRACER, PROGRAM_OCTREE_UPDATE = 0, 1
SHADER_STORAGE_BUFFER, ATOMIC_COUNTER_BUFFER = 0x90D2, 0x92C0

RAY_MISS, RAY_HIT, RAY_ITER_LIMIT = 0, 1, 2
# tdt_ray_hit (include/tdt_rt.h), field for field
RAY_HIT_DTYPE = np.dtype([("status", "<i4"), ("material", "<u4"), ("t", "<f4"), ("iterations", "<i4"),
                          ("point", "<f4", (3,)), ("normal", "<f4", (3,)), ("front_face", "<i4"), ("fresh_record", "<i4"),
                          ("cell_min", "<f4", (3,)), ("cell_size", "<f4")])
assert RAY_HIT_DTYPE.itemsize == 64


def hits_from_bytes(b):
    """(n, 64) uint8 (numpy, or a torch tensor on any device) -> numpy array of RAY_HIT_DTYPE, shape (n,)."""
    if hasattr(b, "detach"):
        b = b.detach().cpu().numpy()
    return np.ascontiguousarray(b, np.uint8).reshape(-1, 64).view(RAY_HIT_DTYPE).reshape(-1)


# guide images and the denoiser (include/tdt_rt.h): the flag and struct tdt_guide_texel, field for field
GUIDE_ALL_MATERIALS = 1
GUIDE_TEXEL_DTYPE = np.dtype([("kind", "<u4"), ("material", "<u4"), ("plane", "<f4"), ("t", "<f4")])
assert GUIDE_TEXEL_DTYPE.itemsize == 16


class VIEW(ctypes.Structure):
    """struct tdt_view: a snapshot of the camera uniforms primary_ray reads (temporal reprojection maps into it)."""
    _fields_ = [("origin", ctypes.c_float * 3), ("lower_left_corner", ctypes.c_float * 3), ("horizontal", ctypes.c_float * 3),
                ("vertical", ctypes.c_float * 3), ("image_width", ctypes.c_int32), ("image_height", ctypes.c_int32)]


assert ctypes.sizeof(VIEW) == 56


# region edits (include/tdt_rt.h): shapes, ops, and struct tdt_region
SHAPE_BOX, SHAPE_SPHERE = 0, 1
REGION_SET, REGION_FILL, REGION_PAINT, REGION_CLEAR = 0, 1, 2, 3
REGION_BRUSH_CAP = 1 << 26


class Region(ctypes.Structure):
    """struct tdt_region: box a = lo, b = hi (inclusive); sphere a = centre, b[0] = radius."""
    _fields_ = [("shape", ctypes.c_int32), ("a", ctypes.c_int32 * 3), ("b", ctypes.c_int32 * 3), ("pad", ctypes.c_int32)]


assert ctypes.sizeof(Region) == 32


def box(lo, hi):
    return Region(SHAPE_BOX, (ctypes.c_int32 * 3)(*[int(v) for v in lo]), (ctypes.c_int32 * 3)(*[int(v) for v in hi]), 0)


def sphere(centre, radius):
    return Region(SHAPE_SPHERE, (ctypes.c_int32 * 3)(*[int(v) for v in centre]), (ctypes.c_int32 * 3)(int(radius), 0, 0), 0)


def _regions(regions):
    """One Region, or a sequence of them -> (ctypes array or None, count)."""
    if isinstance(regions, Region):
        regions = [regions]
    regions = list(regions)
    if not regions:
        return None, 0
    return (Region * len(regions))(*regions), len(regions)


# connected components (include/tdt_rt.h): match rules, struct tdt_select, struct tdt_component
MATCH_ANY, MATCH_MATERIAL = 0, 1
COMPONENT_DTYPE = np.dtype([("first", "<u4"), ("voxels", "<u4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("material", "<i4"),
                            ("pad", "<i4")])
assert COMPONENT_DTYPE.itemsize == 40


class Select(ctypes.Structure):
    """struct tdt_select: connectivity 6 / 26, match MATCH_*, the inclusive size window, invert 0 / 1."""
    _fields_ = [("connectivity", ctypes.c_int32), ("match", ctypes.c_int32), ("min_voxels", ctypes.c_uint32),
                ("max_voxels", ctypes.c_uint32), ("invert", ctypes.c_int32), ("pad", ctypes.c_int32)]


assert ctypes.sizeof(Select) == 24


def _seeds(seeds):
    """None (no seed filter) or (n, 3) voxel coordinates -> (contiguous int32 array or None, count).  An empty sequence is a seed
    filter that matches nothing, not the absence of one (the C ABI reads n_seeds = 0 as "any component"): it becomes one seed
    off the grid, which matches nothing."""
    if seeds is None:
        return None, 0
    s = np.asarray(seeds, np.int32).reshape(-1, 3)
    if not len(s):
        s = np.full((1, 3), -1, np.int32)
    return np.ascontiguousarray(s), len(s)


def _touch_regions(regions):
    """None (no region filter), one Region or a sequence -> (ctypes array or None, count); an empty sequence is a region filter
    that matches nothing (one empty box), as with seeds."""
    if regions is None:
        return None, 0
    arr, k = _regions(regions)
    return _regions(box((0, 0, 0), (-1, -1, -1))) if k == 0 else (arr, k)


# voxel morphology (include/tdt_rt.h): ops and struct tdt_morph
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE, MORPH_SHELL = 0, 1, 2, 3, 4


class Morph(ctypes.Structure):
    """struct tdt_morph: op MORPH_*, connectivity 6 / 26 (one step's structuring element), radius 1..64 steps, material -1
    (inherit) or 0..253, border 0 / 1 (outside the grid empty / solid)."""
    _fields_ = [("op", ctypes.c_int32), ("connectivity", ctypes.c_int32), ("radius", ctypes.c_int32), ("material", ctypes.c_int32),
                ("border", ctypes.c_int32), ("pad", ctypes.c_int32)]


assert ctypes.sizeof(Morph) == 24


# triangle meshes (include/tdt_rt.h): fixed-point vertices (MESH_FRAC fractional bits) and struct tdt_mesh
MESH_FRAC, MESH_COORD_MAX = 6, 1 << 18


class Mesh(ctypes.Structure):
    """struct tdt_mesh: vertices n_vertices x {x, y, z} int32 fixed point, triangles n_triangles x 3 uint32 indices, materials
    n_triangles x (material + 1) int32 or NULL (then `material` 0..253 for every triangle)."""
    _fields_ = [("vertices", ctypes.c_void_p), ("triangles", ctypes.c_void_p), ("materials", ctypes.c_void_p),
                ("n_vertices", ctypes.c_uint32), ("n_triangles", ctypes.c_uint32), ("material", ctypes.c_int32), ("pad", ctypes.c_int32)]


assert ctypes.sizeof(Mesh) == 40


# enclosed space (include/tdt_rt.h): struct tdt_fill
class Fill(ctypes.Structure):
    """struct tdt_fill: connectivity 6 / 26 of the EMPTY voxels, material -1 (inherit along -x) or 0..253."""
    _fields_ = [("connectivity", ctypes.c_int32), ("material", ctypes.c_int32)]


assert ctypes.sizeof(Fill) == 8
assert Fill.connectivity.offset == 0 and Fill.material.offset == 4


# surface extraction (include/tdt_rt.h): struct tdt_surface, struct tdt_quad
class Surface(ctypes.Structure):
    """struct tdt_surface: merge 0 / 1 (one quad per exposed face / runs, then stacks of identical runs), by_material 0 / 1 (faces
    carry 0 / material + 1)."""
    _fields_ = [("merge", ctypes.c_int32), ("by_material", ctypes.c_int32)]


class Quad(ctypes.Structure):
    """struct tdt_quad: face 0..5 (-x, +x, -y, +y, -z, +z), material + 1 (or 0), the minimum corner in lattice coordinates, the
    extent along u = (a + 1) % 3 and v = (a + 2) % 3."""
    _fields_ = [("face", ctypes.c_int32), ("material", ctypes.c_int32), ("origin", ctypes.c_int32 * 3), ("size", ctypes.c_int32 * 2),
                ("pad", ctypes.c_int32)]


assert ctypes.sizeof(Surface) == 8 and ctypes.sizeof(Quad) == 32

# exact Euclidean distance (include/tdt_rt.h): struct tdt_round
ROUND_DOMAIN_CAP = 1 << 28


class Round(ctypes.Structure):
    """struct tdt_round: op MORPH_*, radius2 1..4096 (the squared radius), material -1 (inherit the nearest voxel's) or 0..253,
    border 0 / 1 (outside the grid empty / solid)."""
    _fields_ = [("op", ctypes.c_int32), ("radius2", ctypes.c_int32), ("material", ctypes.c_int32), ("border", ctypes.c_int32)]


assert ctypes.sizeof(Round) == 16

# voxel smoothing (include/tdt_rt.h): modes and struct tdt_smooth
SMOOTH_BOTH, SMOOTH_ADD, SMOOTH_REMOVE = 0, 1, 2
SMOOTH_DOMAIN_CAP = 1 << 28


class Smooth(ctypes.Structure):
    """struct tdt_smooth: radius2 1..225 (the squared radius of the ball), iterations 1..16, threshold 0 (majority) or a Q16
    fraction 1..65536 of the support, mode SMOOTH_*, material -1 (inherit the nearest voxel's) or 0..253, border 0 / 1 (outside
    the grid empty / left out of the vote)."""
    _fields_ = [("radius2", ctypes.c_int32), ("iterations", ctypes.c_int32), ("threshold", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("material", ctypes.c_int32), ("border", ctypes.c_int32)]


assert ctypes.sizeof(Smooth) == 24


# affine transforms of voxel selections (include/tdt_rt.h): struct tdt_xform
XFORM_ONE = 65536


class Xform(ctypes.Structure):
    """struct tdt_xform: the destination -> source map s = (a (2 p + 1) + t) >> 17: t three int64 in units of 2^-17 voxel, a nine
    int32 row-major in Q16 (XFORM_ONE = 1.0), material -1 (the source voxel's) or 0..253, dst_lo / dst_hi the inclusive box the
    result is clipped to, pad 0.  host.xform_* build one from a forward transform."""
    _fields_ = [("t", ctypes.c_int64 * 3), ("a", ctypes.c_int32 * 9), ("material", ctypes.c_int32), ("dst_lo", ctypes.c_int32 * 3),
                ("dst_hi", ctypes.c_int32 * 3), ("pad", ctypes.c_int32 * 2)]


assert ctypes.sizeof(Xform) == 96

# geodesic distance (include/tdt_rt.h): media, step-weight presets and struct tdt_geodesic
MEDIUM_EMPTY, MEDIUM_SOLID = 0, 1
GEODESIC_DOMAIN_CAP = 1 << 27
STEPS_6, STEPS_26, CHAMFER_345 = (1, 0, 0), (1, 1, 1), (3, 4, 5)


class Geodesic(ctypes.Structure):
    """struct tdt_geodesic: medium MEDIUM_*, match -1 (any voxel) or 0..253 (SOLID: that LEAF value only), w the cost of a face /
    edge / corner step (w[0] 1..255, the others 0..255 with 0 = no such step), max_cost 0..2^30, material -1 (the voxel's own,
    SOLID only) or 0..253 for the list and edit forms, pad 0."""
    _fields_ = [("medium", ctypes.c_int32), ("match", ctypes.c_int32), ("w", ctypes.c_int32 * 3), ("max_cost", ctypes.c_int32),
                ("material", ctypes.c_int32), ("pad", ctypes.c_int32)]


assert ctypes.sizeof(Geodesic) == 32


def _exact_ints(a, dtype, name):
    """a as a contiguous array of an integer dtype, refusing what the cast would change (a wrapped index would be a valid one)."""
    src = np.asarray(a)
    if src.size and src.dtype.kind not in "iu":
        raise ValueError(f"{name} must be integers, not {src.dtype}")
    out = np.ascontiguousarray(src.astype(dtype))
    if src.size and not np.array_equal(out.astype(object), src.astype(object)):
        raise ValueError(f"{name} holds values outside {np.dtype(dtype).name}")
    return out


def _mesh(vertices, triangles, materials, material):
    """(struct tdt_mesh, the arrays it points into) from (n, 3) fixed-point vertices, (m, 3) vertex indices, None or (m,)
    per-triangle material + 1, and the material used without them.  The ranges are the library's to check."""
    v = _exact_ints(vertices, np.int32, "vertices")
    t = _exact_ints(triangles, np.uint32, "triangles")
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("vertices and triangles must be (n, 3) arrays")
    m = None
    if materials is not None:
        m = _exact_ints(materials, np.int32, "materials").reshape(-1)
        if len(m) != len(t):
            raise ValueError(f"{len(m)} materials for {len(t)} triangles")
    if isinstance(material, bool) or int(material) != material or not -2**31 <= int(material) <= 2**31 - 1:
        raise ValueError(f"material must be an int32, not {material!r}")
    mesh = Mesh(v.ctypes.data if len(v) else None, t.ctypes.data if len(t) else None, m.ctypes.data if m is not None and len(m) else None,
                len(v), len(t), int(material), 0)
    return mesh, (v, t, m)


# stroke brushes (include/tdt_rt.h): the limits of a stroke's points and radius, and struct tdt_stroke
STROKE_COORD_MAX, STROKE_RADIUS_MAX = 8192, 2048


class Stroke(ctypes.Structure):
    """struct tdt_stroke: points n_points x {x, y, z} int32 voxel coordinates, segments n_segments x {i, j} uint32 point indices or
    NULL (the polyline of the points), materials per segment (material + 1) int32 or NULL (then `material` 0..253 for every
    segment), shape SHAPE_SPHERE (round nib) / SHAPE_BOX (cube nib of half-width radius), radius 0..STROKE_RADIUS_MAX, pad 0."""
    _fields_ = [("points", ctypes.c_void_p), ("segments", ctypes.c_void_p), ("materials", ctypes.c_void_p),
                ("n_points", ctypes.c_uint32), ("n_segments", ctypes.c_uint32), ("shape", ctypes.c_int32), ("radius", ctypes.c_int32),
                ("material", ctypes.c_int32), ("pad", ctypes.c_int32)]


assert ctypes.sizeof(Stroke) == 48


def _stroke(points, radius, segments=None, materials=None, material=0, shape=SHAPE_SPHERE, depth=None, op=None):
    """(struct tdt_stroke, the arrays it points into) from (n, 3) voxel coordinates, the nib's radius, None (the polyline of the
    points) or (m, 2) point indices, None or per-segment material + 1, the material used without them, and the nib's shape; depth
    / op: those of the call, when it takes them.  What ctypes would wrap or truncate silently is refused, and every range the
    header lists under its errors is checked here as the library checks it (ValueError), so a bad stroke fails before any
    device work; the two 2^26 limits, which depend on the grid, stay the library's."""
    p = _exact_ints(points, np.int32, "points")
    if p.size == 0:
        p = p.reshape(0, 3)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be an (n, 3) array")
    g = None
    if segments is not None:
        g = _exact_ints(segments, np.uint32, "segments")
        if g.size == 0:
            g = g.reshape(0, 2)
        if g.ndim != 2 or g.shape[1] != 2:
            raise ValueError("segments must be an (m, 2) array")
    n_seg = len(g) if g is not None else (len(p) - 1 if len(p) > 1 else len(p))
    m = None
    if materials is not None:
        m = _exact_ints(materials, np.int32, "materials").reshape(-1)
        if len(m) != n_seg:
            raise ValueError(f"{len(m)} materials for {n_seg} segments")
    for name, v, lo, hi in (("radius", radius, 0, STROKE_RADIUS_MAX), ("material", material, 0, 253), ("shape", shape, SHAPE_BOX, SHAPE_SPHERE),
                            ("depth", depth, 1, 10), ("op", op, REGION_SET, REGION_CLEAR)):
        if v is None and name in ("depth", "op"):
            continue
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer, not {v!r}")
        if not lo <= int(v) <= hi and not (name == "material" and m is not None and -2**31 <= int(v) <= 2**31 - 1):
            raise ValueError(f"{name} must be {lo}..{hi}, not {v!r}")
    if len(p) > 1 << 20 or n_seg > 1 << 20:
        raise ValueError("a stroke takes at most 2^20 points and 2^20 segments")
    if p.size and int(np.abs(p.astype(np.int64)).max()) > STROKE_COORD_MAX:
        raise ValueError(f"a point coordinate beyond +-{STROKE_COORD_MAX}")
    if g is not None and g.size and int(g.max()) >= len(p):
        raise ValueError(f"a segment names point {int(g.max())} of {len(p)}")
    if m is not None and m.size and not (1 <= int(m.min()) and int(m.max()) <= 254):
        raise ValueError("materials (material + 1) must be 1..254")
    n_list = len(g) if g is not None else 0
    if g is not None and len(g) == 0:
        g = np.zeros((1, 2), np.uint32)                # an explicit empty list still needs an address: NULL means the polyline
    stroke = Stroke(p.ctypes.data if len(p) else None, g.ctypes.data if g is not None else None,
                    m.ctypes.data if m is not None and len(m) else None, len(p), n_list, int(shape), int(radius), int(material), 0)
    return stroke, (p, g, m)


# face tools (include/tdt_rt.h): struct tdt_faces, struct tdt_face_region, the distance limit and what extract_faces lists
FACES_DISTANCE_MAX = 1023
FACES_COLUMNS, FACES_TREE = 0, 1


class Faces(ctypes.Structure):
    """struct tdt_faces: connectivity 4 / 8 of the exposed faces inside a plane, match MATCH_*, the signed distance
    -FACES_DISTANCE_MAX..FACES_DISTANCE_MAX (> 0 pulls, < 0 pushes), block 0 / 1 (stop at an obstacle / at the air behind),
    material -1 (inherit the face's) or 0..253, pad 0."""
    _fields_ = [("connectivity", ctypes.c_int32), ("match", ctypes.c_int32), ("distance", ctypes.c_int32), ("block", ctypes.c_int32),
                ("material", ctypes.c_int32), ("pad", ctypes.c_int32)]


class FaceRegion(ctypes.Structure):
    """struct tdt_face_region: the index in F of its first face, its size, its direction 0..5 and the voxels' own coordinate along
    the axis, the inclusive (u, v) bounding box, the carried material (material + 1) of its first face."""
    _fields_ = [("first", ctypes.c_uint32), ("faces", ctypes.c_uint32), ("face", ctypes.c_int32), ("w", ctypes.c_int32),
                ("lo", ctypes.c_int32 * 2), ("hi", ctypes.c_int32 * 2), ("material", ctypes.c_int32), ("pad", ctypes.c_int32)]


FACE_REGION_DTYPE = np.dtype([("first", "<u4"), ("faces", "<u4"), ("face", "<i4"), ("w", "<i4"), ("lo", "<i4", (2,)), ("hi", "<i4", (2,)),
                              ("material", "<i4"), ("pad", "<i4")])
assert ctypes.sizeof(Faces) == 24 and ctypes.sizeof(FaceRegion) == 40 == FACE_REGION_DTYPE.itemsize


def _faces(seeds, distance, connectivity=4, match=MATCH_MATERIAL, block=False, material=-1, what=None, op=None):
    """(struct tdt_faces, the contiguous (n, 4) int32 seed array {x, y, z, f}) for the face tools; what / op: those of the call,
    when it takes them.  What ctypes would wrap or truncate silently is refused, and every range the header lists under its errors
    is checked here as the library checks it (ValueError), so a bad call fails before any device work; the 2^26 limits, which
    depend on the tree, stay the library's.  block takes True / False; everything else must be an integer."""
    s = _exact_ints(seeds, np.int32, "seeds")
    if s.size == 0:
        s = s.reshape(0, 4)
    if s.ndim == 1 and s.size == 4:
        s = s.reshape(1, 4)
    if s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("seeds must be an (n, 4) array of {x, y, z, f}")
    if len(s) > 1 << 20:
        raise ValueError("the face tools take at most 2^20 seeds")
    if len(s) and not (0 <= int(s[:, 3].min()) and int(s[:, 3].max()) <= 5):
        raise ValueError("a seed's face must be 0..5")
    if isinstance(block, (bool, np.bool_)):
        block = int(block)
    for name, v, allowed in (("connectivity", connectivity, (4, 8)), ("match", match, (MATCH_ANY, MATCH_MATERIAL)),
                             ("distance", distance, range(-FACES_DISTANCE_MAX, FACES_DISTANCE_MAX + 1)), ("block", block, (0, 1)),
                             ("material", material, range(-1, 254)), ("what", what, (FACES_COLUMNS, FACES_TREE)),
                             ("op", op, range(REGION_SET, REGION_CLEAR + 1))):
        if v is None and name in ("what", "op"):
            continue
        if isinstance(v, (bool, np.bool_)) or v is None or int(v) != v:
            raise ValueError(f"{name} must be an integer, not {v!r}")
        if int(v) not in allowed:
            raise ValueError(f"{name} must be one of {allowed!r}, not {v!r}")
    return Faces(int(connectivity), int(match), int(distance), int(block), int(material), 0), np.ascontiguousarray(s)


class Adapt(ctypes.Structure):
    """struct tdt_adapt: the relative error of the mean luminance at which a pixel stops, the brightness floor that error is
    measured against, and the fewest / most samples a pixel receives."""
    _fields_ = [("tolerance", ctypes.c_float), ("floor", ctypes.c_float), ("min_samples", ctypes.c_int32), ("max_samples", ctypes.c_int32)]


assert ctypes.sizeof(Adapt) == 16

OVERLAY_VOXEL_EDGES = 1
VOXEL_ID_TEXEL_DTYPE = np.dtype([("state", "<u4"), ("key", "<u4"), ("material", "<u4"), ("t", "<u4")])
assert VOXEL_ID_TEXEL_DTYPE.itemsize == 16


class Overlay(ctypes.Structure):
    """struct tdt_overlay: the colours (r, g, b, a) of member and of edge pixels, the outline's width in pixels (0..4, 0 = none)
    and the flags (OVERLAY_VOXEL_EDGES: outline every voxel, not only the selection's silhouette)."""
    _fields_ = [("fill", ctypes.c_float * 4), ("edge", ctypes.c_float * 4), ("edge_width", ctypes.c_int32), ("flags", ctypes.c_uint32)]


assert ctypes.sizeof(Overlay) == 40


def _overlay(fill, edge, edge_width, voxel_edges):
    """The Overlay of Texture.overlay's arguments, refused here where they are not what the struct can carry."""
    fill = tuple(float(v) for v in fill)
    edge = fill if edge is None else tuple(float(v) for v in edge)
    if len(fill) != 4 or len(edge) != 4:
        raise ValueError("overlay: fill and edge are (r, g, b, a)")
    if isinstance(edge_width, bool) or not isinstance(edge_width, (int, np.integer)) or not 0 <= edge_width <= 4:
        raise ValueError("overlay: edge_width must be an int 0..4")
    return Overlay((ctypes.c_float * 4)(*fill), (ctypes.c_float * 4)(*edge), int(edge_width), OVERLAY_VOXEL_EDGES if voxel_edges else 0)


def _place(place):
    if isinstance(place, bool) or place not in (0, 1):
        raise ValueError("place must be 1 (the empty cell in front of the face) or 0 (the voxel behind it)")
    return int(place)


# through-selection (include/tdt_rt.h): shapes, the flag and struct tdt_screen_select
SCREEN_RECT, SCREEN_POLYGON, SCREEN_MASK = 0, 1, 2
SCREEN_WINDOW = 1
SCREEN_MAX_VERTICES = 256


class ScreenSelect(ctypes.Structure):
    """struct tdt_screen_select: the shape (SCREEN_*), rect = (x0, y0, x1, y1) inclusive (SCREEN_RECT only), the flags
    (SCREEN_WINDOW: all eight corners of a voxel must pass, not its centre), the material filter (-1: any) and the distance range
    from the view's origin (0 and inf: no limit)."""
    _fields_ = [("shape", ctypes.c_int32), ("rect", ctypes.c_int32 * 4), ("flags", ctypes.c_uint32), ("material", ctypes.c_int32),
                ("min_distance", ctypes.c_float), ("max_distance", ctypes.c_float)]


assert ctypes.sizeof(ScreenSelect) == 36


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _screen_select(rect, polygon, mask, window, material, min_distance, max_distance):
    """(ScreenSelect, polygon as a contiguous (n, 2) int32 array or None, mask) of the arguments every through-selection call takes,
    refused here where they are not what the C ABI can carry."""
    if sum(a is not None for a in (rect, polygon, mask)) != 1:
        raise ValueError("through-selection takes exactly one of rect, polygon and mask")
    if not isinstance(window, (bool, np.bool_)):
        raise ValueError("window must be a bool")
    if material is not None and (not _is_int(material) or not 0 <= material <= 253):
        raise ValueError("material must be None (any) or an int 0..253")
    lo, hi = float(min_distance), float(max_distance)
    if not (0.0 <= lo <= hi):
        raise ValueError("the distances must be 0 <= min_distance <= max_distance")
    sel = ScreenSelect(SCREEN_RECT, (ctypes.c_int32 * 4)(), SCREEN_WINDOW if window else 0, -1 if material is None else int(material), lo, hi)
    pts = None
    if rect is not None:
        if len(rect) != 4 or not all(_is_int(v) and abs(v) < 2**31 for v in rect):
            raise ValueError("rect is four ints (x0, y0, x1, y1)")
        sel.rect = (ctypes.c_int32 * 4)(*[int(v) for v in rect])
    elif polygon is not None:
        p = np.asarray(polygon)
        if p.ndim != 2 or p.shape[1] != 2 or not 3 <= len(p) <= SCREEN_MAX_VERTICES or p.dtype.kind not in "iu" or np.abs(p.astype(np.int64)).max() > 1 << 20:
            raise ValueError("polygon is 3..256 integer vertices (x, y), each coordinate within +-2^20")
        sel.shape = SCREEN_POLYGON
        pts = np.ascontiguousarray(p, np.int32)
    else:
        if not isinstance(mask, Texture):
            raise ValueError("mask is a Texture of the view's size")
        sel.shape = SCREEN_MASK
    return sel, pts, mask

# every symbol include/tdt_rt.h declares: (name, restype, argtypes)
_P, _I, _U, _F, _S = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_size_t
_PP = ctypes.POINTER(ctypes.c_void_p)
SYMBOLS = [
    ("tdt_ctx_create", _I, [_I, _P, _PP]),
    ("tdt_ctx_create_multi", _I, [_I, ctypes.POINTER(ctypes.c_int), _PP]),
    ("tdt_ctx_device_count", _I, [_P]),
    ("tdt_ctx_destroy", None, [_P]),
    ("tdt_finish", _I, [_P]),
    ("tdt_last_error", ctypes.c_char_p, [_P]),
    ("tdt_strerror", ctypes.c_char_p, [_I]),
    ("tdt_compute_create", _I, [_P, _I, _PP]),
    ("tdt_compute_destroy", None, [_P]),
    ("tdt_compute_group_size", _I, [_P, ctypes.POINTER(ctypes.c_int)]),
    ("tdt_set_i32", _I, [_P, ctypes.c_char_p, ctypes.c_int32]),
    ("tdt_set_f32", _I, [_P, ctypes.c_char_p, _F]),
    ("tdt_set_vec3f", _I, [_P, ctypes.c_char_p, _F, _F, _F]),
    ("tdt_set_vec3i", _I, [_P, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    ("tdt_buffer_create", _I, [_P, _P, _S, _PP]),
    ("tdt_buffer_destroy", None, [_P]),
    ("tdt_bind_buffer_base", _I, [_P, _I, _U, _P]),
    ("tdt_buffer_sub_data", _I, [_P, _S, _S, _P]),
    ("tdt_buffer_read", _I, [_P, _S, _S, _P]),
    ("tdt_image_create_rgba32f", _I, [_P, _I, _I, _PP]),
    ("tdt_image_wrap_device", _I, [_P, _P, _I, _I, _PP]),
    ("tdt_image_destroy", None, [_P]),
    ("tdt_bind_image", _I, [_P, _U, _P]),
    ("tdt_image_width", _I, [_P]),
    ("tdt_image_height", _I, [_P]),
    ("tdt_image_device_ptr", _P, [_P]),
    ("tdt_image_read", _I, [_P, _P]),
    ("tdt_image_read_rgba8", _I, [_P, _I, _P]),
    ("tdt_dispatch_compute", _I, [_P, _I, _I, _I]),
    ("tdt_set_partition", _I, [_P, _I, _I]),
    ("tdt_dispatch_accumulate", _I, [_P, _I, _I, _I, _I, _I, _P]),
    ("tdt_dispatch_accumulate_masked", _I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    ("tdt_dispatch_resolve", _I, [_P, _I, _I, _I, _I]),
    ("tdt_covered_pixels", ctypes.c_int64, [_P, _I, _I, _I]),
    ("tdt_owned_tiles", _I, [_P, _I, _I, _I, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("tdt_assemble_tiles", _I, [_P, _P, _I, _I, _P, _I, _I, _I]),
    ("tdt_dispatch_counted", _I, [_P, _I, _I, _I, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_dispatch_counted_range", _I, [_P, _I, _I, _I, _I, _I, _P, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_forget_costs", _I, [_P]),
    ("tdt_debug_phase_timing", _I, [_P, _I, ctypes.POINTER(ctypes.c_float)]),
    ("tdt_debug_multi_timing", _I, [_P, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    ("tdt_debug_multi_transport", ctypes.c_char_p, [_P]),
    ("tdt_debug_multi_rccl_ranks", _I, [_P]),
    ("tdt_debug_multi_fail", _I, [_P, _I]),
    ("tdt_octree_build_cells", _I, [_P, _P, _S, _I, _PP, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_build_from_points", _I, [_P, _P, _S, ctypes.POINTER(ctypes.c_int32), _P, _P, _S, _I, _I, _PP,
                                          ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    ("tdt_debug_edit_mode", _I, [_P, _I]),
    ("tdt_debug_last_edit_path", _I, [_P]),
    ("tdt_debug_last_variant", _I, [_P, ctypes.POINTER(ctypes.c_int)]),
    ("tdt_debug_last_geometry", _I, [_P, ctypes.POINTER(ctypes.c_int)]),
    ("tdt_debug_trace_variants", _I, [ctypes.POINTER(ctypes.c_int), _I, ctypes.POINTER(ctypes.c_int)]),
    ("tdt_debug_counters", _I, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_debug_stats", _I, [_P, ctypes.POINTER(ctypes.c_uint64), _I, _I]),
    ("tdt_debug_wave_ends", _I, [_P, ctypes.POINTER(ctypes.c_uint64), _I]),
    ("tdt_debug_pixel_log", _I, [_P, ctypes.c_void_p, ctypes.c_size_t]),
    ("tdt_raycast", _I, [_P, _P, _S, _P]),
    ("tdt_raycast_device", _I, [_P, _P, _S, _P]),
    ("tdt_pick_pixels", _I, [_P, _P, _S, _I, _P, _P]),
    ("tdt_dispatch_guide", _I, [_P, _P, _I, ctypes.c_uint32]),
    ("tdt_image_denoise", _I, [_P, _P, _I, ctypes.c_uint32]),
    ("tdt_compute_view", _I, [_P, ctypes.POINTER(VIEW)]),
    ("tdt_image_reproject", _I, [_P, _I, _P, _P, _I, ctypes.POINTER(VIEW), _P, _P, _F, _P, _P, ctypes.c_uint32]),
    ("tdt_debug_reproject_counts", _I, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_image_clear", _I, [_P]),
    ("tdt_image_variance", _I, [_P, _P, _P, _F, ctypes.c_uint32]),
    ("tdt_image_denoise_variance", _I, [_P, _P, _I, _F, _F, ctypes.c_uint32]),
    ("tdt_image_reproject_moments", _I, [_P, _I, _P, _P, _I, ctypes.POINTER(VIEW), _P, _P, _P, _F, _P, _P, _P, ctypes.c_uint32]),
    ("tdt_image_upsample", _I, [_P, _P, _P, _P, ctypes.c_uint32]),
    ("tdt_debug_upsample_counts", _I, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_image_adapt", _I, [_P, _P, _P, _P, _I, ctypes.POINTER(Adapt), ctypes.c_uint32]),
    ("tdt_debug_adapt_counts", _I, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_image_adapt_mean", _I, [_P, _P, ctypes.c_uint32]),
    ("tdt_dispatch_voxel_ids", _I, [_P, _P, _I, _I]),
    ("tdt_image_overlay", _I, [_P, _P, _P, _S, ctypes.POINTER(Overlay)]),
    ("tdt_debug_overlay_counts", _I, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_image_extract_voxels", _I, [_P, ctypes.POINTER(ctypes.c_int32), _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_extract_screen", _I, [_P, ctypes.POINTER(VIEW), ctypes.POINTER(ScreenSelect), _P, _S, _P, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_edit_screen", _I, [_P, _I, ctypes.POINTER(VIEW), ctypes.POINTER(ScreenSelect), _P, _S, _P, ctypes.c_int32,
                                    ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_debug_screen_counts", _I, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_octree_census", _I, [_P, ctypes.POINTER(ctypes.c_int64)]),
    ("tdt_octree_extract", _I, [_P, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_compact", _I, [_P, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_edit_region", _I, [_P, _I, _P, _S, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_edit_voxels", _I, [_P, _I, _P, _S, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_extract_region", _I, [_P, _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_components", _I, [_P, _I, _I, _P, _S, ctypes.POINTER(ctypes.c_size_t), _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_edit_connected", _I, [_P, _I, ctypes.POINTER(Select), _P, _S, _P, _S, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_extract_connected", _I, [_P, ctypes.POINTER(Select), _P, _S, _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_morph", _I, [_P, ctypes.POINTER(Morph), _P, _S, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_extract_morph", _I, [_P, ctypes.POINTER(Morph), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_voxelize_triangles", _I, [_P, ctypes.POINTER(Mesh), _I, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_edit_triangles", _I, [_P, _I, ctypes.POINTER(Mesh), ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_voxelize_stroke", _I, [_P, ctypes.POINTER(Stroke), _I, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_edit_stroke", _I, [_P, _I, ctypes.POINTER(Stroke), ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_extract_stroke", _I, [_P, ctypes.POINTER(Stroke), _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_extract_enclosed", _I, [_P, ctypes.POINTER(Fill), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_fill_enclosed", _I, [_P, ctypes.POINTER(Fill), _P, _S, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_voxelize_triangles_solid", _I, [_P, ctypes.POINTER(Mesh), _I, ctypes.POINTER(Fill), _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_edit_triangles_solid", _I, [_P, _I, ctypes.POINTER(Mesh), ctypes.POINTER(Fill), ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_debug_fill_passes", _I, [_P]),
    ("tdt_octree_extract_surface", _I, [_P, ctypes.POINTER(Surface), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_face_regions", _I, [_P, _I, _I, _P, _S, _P, _P, _S, ctypes.POINTER(ctypes.c_size_t), _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_extract_faces", _I, [_P, ctypes.POINTER(Faces), _P, _S, _P, _S, _I, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_edit_faces", _I, [_P, _I, ctypes.POINTER(Faces), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_debug_faces_premerge", _I, [_P, _I]),
    ("tdt_octree_morph_round", _I, [_P, ctypes.POINTER(Round), _P, _S, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_extract_morph_round", _I, [_P, ctypes.POINTER(Round), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_distance_field", _I, [_P, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32,
                                       _P, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_ball_size", ctypes.c_int32, [ctypes.c_int32]),
    ("tdt_octree_smooth", _I, [_P, ctypes.POINTER(Smooth), _P, _S, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_extract_smooth", _I, [_P, ctypes.POINTER(Smooth), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_density_field", _I, [_P, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, _P, _P, _S,
                                      ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_extract_transform", _I, [_P, ctypes.POINTER(Xform), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_transform", _I, [_P, ctypes.POINTER(Xform), _I, _P, _S, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_debug_xform_bricks", _I, [_P, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_geodesic_field", _I, [_P, ctypes.POINTER(Geodesic), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                       _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_extract_geodesic", _I, [_P, ctypes.POINTER(Geodesic), _P, _S, _P, _S, _P, _S, ctypes.POINTER(ctypes.c_size_t)]),
    ("tdt_octree_edit_geodesic", _I, [_P, _I, ctypes.POINTER(Geodesic), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_uint32)]),
    ("tdt_octree_geodesic_path", _I, [_P, ctypes.POINTER(Geodesic), _P, _S, _P, _S, ctypes.POINTER(ctypes.c_int32), _P, _S,
                                      ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]),
    ("tdt_debug_geodesic_passes", _I, [_P]),
    ("tdt_selftest", _I, [_P, _I, ctypes.POINTER(ctypes.c_uint64)]),
    ("tdt_selftest_index", _I, [_P, ctypes.c_int32, _F, ctypes.c_uint32, _I, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]),
]

_lib = None


def lib():
    """Load libtdtrt.so (raises if it has not been built: there is no other implementation)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                               "the trace has no CPU fallback")
        # One HIP runtime per process: PyTorch bundles its own libamdhip64; if ours (from /opt/rocm) were
        # loaded first, torch would later find "no HIP GPUs".  Importing torch first makes both share one.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            try:
                f = getattr(L, name)
            except AttributeError:
                if os.environ.get("TDT_LIB"):                # an older build loaded for an A/B run: newer entry points are absent
                    continue
                raise
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def ball_size(radius2):
    """tdt_ball_size: the number of lattice points d with |d|^2 <= radius2, for 1..4096; -1 otherwise.  Host arithmetic: no device."""
    if isinstance(radius2, bool) or int(radius2) != radius2 or not -2**31 <= int(radius2) <= 2**31 - 1:
        raise ValueError(f"radius2 must be an int32, not {radius2!r}")
    return int(lib().tdt_ball_size(int(radius2)))


class TdtError(RuntimeError):
    """InitializeErr (renderer/mod.rs:28-33) analogue: carries the integer code of the C ABI."""

    def __init__(self, code, message):
        super().__init__(f"[{code:#x}] {message}")
        self.code = code


class Context:
    """The GL context of main.rs:58-61,108-112: one HIP device + stream."""

    def __init__(self, device=0, stream=None, devices=None):
        """devices = [ids]: ONE context over several GPUs (tdt_ctx_create_multi): uploads replicate, a raytracer dispatch is
        sharded over the devices and gathered + assembled on the first; otherwise a single-device context."""
        h = ctypes.c_void_p()
        if devices is not None:
            ids = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
            rc = lib().tdt_ctx_create_multi(len(devices), ids, ctypes.byref(h))
            device = devices[0] if len(devices) else 0
        else:
            rc = lib().tdt_ctx_create(int(device), ctypes.c_void_p(stream) if stream else None, ctypes.byref(h))
        if rc != OK:
            raise TdtError(rc, lib().tdt_last_error(None).decode())
        self.h = h
        self.device = device

    def device_count(self):
        return int(lib().tdt_ctx_device_count(self.h))

    def forget_costs(self):
        """Drop the per-pixel cost history: the next dispatch_compute is scheduled like a context's first frame."""
        self.check(lib().tdt_forget_costs(self.h))

    def phase_timing(self, enable=True):
        """(probe_ms, main_ms, resolve_ms) of the last dispatch_compute (blocks); switches the recording on / off."""
        ms = (ctypes.c_float * 3)()
        self.check(lib().tdt_debug_phase_timing(self.h, 1 if enable else 0, ms))
        return tuple(float(v) for v in ms)

    def multi_timing(self):
        """Multi-device context: ([trace ms per device], gather ms, assemble ms) of the last raytracer dispatch (blocks)."""
        n = self.device_count()
        tr, g, a = (ctypes.c_float * n)(), ctypes.c_float(), ctypes.c_float()
        self.check(lib().tdt_debug_multi_timing(self.h, tr, ctypes.byref(g), ctypes.byref(a)))
        return [float(v) for v in tr], float(g.value), float(a.value)

    def multi_transport(self):
        return lib().tdt_debug_multi_transport(self.h).decode()

    def multi_rccl_ranks(self):
        """Ranks of the RCCL communicator a multi-device context created (0: none / copy transport)."""
        return int(lib().tdt_debug_multi_rccl_ranks(self.h))

    def multi_fail(self, member):
        """Test hook: the next raytracer dispatch fails at device index `member` (after the devices before it were launched)."""
        self.check(lib().tdt_debug_multi_fail(self.h, int(member)))

    def edit_mode(self, mode):
        """0: edits run in parallel when that is provably the ordered result; 1: always the ordered one-lane walk."""
        self.check(lib().tdt_debug_edit_mode(self.h, mode))

    def last_edit_path(self):
        """1 = the last edit dispatch took the ordered walk, 2 = the parallel form, 0 = none yet."""
        return int(lib().tdt_debug_last_edit_path(self.h))

    def check(self, rc):
        if rc != OK:
            raise TdtError(rc, lib().tdt_last_error(self.h).decode() or lib().tdt_strerror(rc).decode())

    def finish(self):
        self.check(lib().tdt_finish(self.h))

    def raycast(self, rays):
        """tdt_raycast: (n, 6) rays {origin, direction} (normalised directions: the traversal step is in units of t) through the
        bound octree (slots 0, 6, 7).  A numpy array -> numpy array of RAY_HIT_DTYPE; a torch tensor on the GPU (float32, (n, 6),
        on the context's first device) -> a (n, 64) uint8 tensor on that device (tdt_raycast_device; hits_from_bytes reads
        it), after torch's pending work on the device and the query have finished."""
        if hasattr(rays, "data_ptr") and getattr(rays, "is_cuda", False):
            import torch
            r = rays.detach().to(torch.float32).contiguous().reshape(-1, 6)
            out = torch.empty((r.shape[0], 64), dtype=torch.uint8, device=r.device)
            torch.cuda.synchronize(r.device)
            self.check(lib().tdt_raycast_device(self.h, ctypes.c_void_p(r.data_ptr()), r.shape[0], ctypes.c_void_p(out.data_ptr())))
            self.finish()
            return out
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros(r.shape[0], RAY_HIT_DTYPE)
        self.check(lib().tdt_raycast(self.h, r.ctypes.data, r.shape[0], out.ctypes.data))
        return out

    CENSUS_FIELDS = ("reachable_cells", "leaf_nodes", "voxels", "max_cell", "buffer_cells", "counter")

    def octree_census(self):
        """tdt_octree_census: what a walk of the bound tree (slots 0, 7) reaches, as a dict of CENSUS_FIELDS; counter = the first word
        of the atomic counter, -1 when none is bound."""
        out = (ctypes.c_int64 * 6)()
        self.check(lib().tdt_octree_census(self.h, out))
        return dict(zip(self.CENSUS_FIELDS, [int(v) for v in out]))

    def _list(self, fn, *args, width=4, tail=()):
        """The two-call list protocol of fn(ctx, *args, array, capacity, &n, *tail): a call without an array for the count, then an
        (n, width) int32 array that a second call fills when n > 0."""
        n = ctypes.c_size_t(0)
        self.check(fn(self.h, *args, None, 0, ctypes.byref(n), *tail))
        out = np.zeros((n.value, width), np.int32)
        if n.value:
            self.check(fn(self.h, *args, out.ctypes.data, n.value, ctypes.byref(n), *tail))
        return out

    def octree_extract(self):
        """tdt_octree_extract: the bound tree's voxels as an (n, 4) int32 array {x, y, z, material + 1}, sorted by Morton key."""
        return self._list(lib().tdt_octree_extract)

    def octree_compact(self):
        """tdt_octree_compact: rewrite the bound cells buffer in place into the canonical tree of its voxels; returns its cell count."""
        n = ctypes.c_uint32(0)
        self.check(lib().tdt_octree_compact(self.h, ctypes.byref(n)))
        return int(n.value)

    def _check_edit(self, rc, n):
        """check() for the region edits: a TdtError carries n_cells, the cell count a too-small buffer would need (else 0)."""
        try:
            self.check(rc)
        except TdtError as e:
            e.n_cells = int(n.value)
            raise

    def octree_edit_region(self, op, regions, material=0):
        """tdt_octree_edit_region: op (REGION_*) over the union of `regions` (one Region or a list; see box / sphere) with brush
        material 0..253, rebuilding the bound tree in place; returns the canonical tree's cell count."""
        arr, k = _regions(regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_region(self.h, int(op), arr, k, int(material), ctypes.byref(n)), n)
        return int(n.value)

    def octree_edit_voxels(self, op, voxels):
        """tdt_octree_edit_voxels: op over an (n, 4) int32 voxel list {x, y, z, m} (m = material + 1; last duplicate wins,
        voxels off the grid are dropped); returns the canonical tree's cell count."""
        v = np.ascontiguousarray(np.asarray(voxels, np.int32).reshape(-1, 4))
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_voxels(self.h, int(op), v.ctypes.data if len(v) else None, len(v), ctypes.byref(n)), n)
        return int(n.value)

    def octree_extract_region(self, regions):
        """tdt_octree_extract_region: the bound tree's voxels inside the union of `regions`, (n, 4) int32, Morton-sorted."""
        arr, k = _regions(regions)
        return self._list(lib().tdt_octree_extract_region, arr, k)

    def _voxel_count(self):
        """The bound tree's voxel count from a walk alone (tdt_octree_extract with a null array), without labelling anything."""
        n = ctypes.c_size_t(0)
        self.check(lib().tdt_octree_extract(self.h, None, 0, ctypes.byref(n)))
        return n.value

    def octree_components(self, connectivity=6, match=MATCH_ANY, capacity=4096):
        """tdt_octree_components: (labels, components) of the bound tree's voxels — labels (n,) uint32 in octree_extract's order,
        components a COMPONENT_DTYPE array numbered in the Morton order of each component's first voxel.  A count query would cost a
        whole labelling, so this labels once: the labels are sized by a walk, the table by `capacity`, and only a tree of more
        components than that is labelled a second time, into a table of the size the first call reported."""
        nv, nc = ctypes.c_size_t(0), ctypes.c_size_t(0)
        labels = np.zeros(self._voxel_count(), np.uint32)
        comps = np.zeros(max(int(capacity), 1), COMPONENT_DTYPE)

        def run():
            return lib().tdt_octree_components(self.h, int(connectivity), int(match), labels.ctypes.data, len(labels), ctypes.byref(nv),
                                               comps.ctypes.data, len(comps), ctypes.byref(nc))

        rc = run()
        if rc == ERR_INVALID_VALUE and (nv.value > len(labels) or nc.value > len(comps)):
            labels = np.zeros(nv.value, np.uint32)
            comps = np.zeros(nc.value, COMPONENT_DTYPE)
            rc = run()
        self.check(rc)
        return labels, comps[: nc.value].copy()

    @staticmethod
    def _select(connectivity, match, min_voxels, max_voxels, invert):
        """struct tdt_select; the size window must be 0 .. 2^32 - 1 (ctypes would wrap a negative value silently)."""
        for name, v in (("min_voxels", min_voxels), ("max_voxels", max_voxels)):
            if not 0 <= int(v) <= 2**32 - 1:
                raise ValueError(f"{name} must be 0 .. 2^32 - 1, not {v}")
        return Select(int(connectivity), int(match), int(min_voxels), int(max_voxels), int(invert), 0)

    def octree_edit_connected(self, op, seeds=None, regions=None, connectivity=6, match=MATCH_ANY, min_voxels=0, max_voxels=2**32 - 1,
                              invert=False, material=0):
        """tdt_octree_edit_connected: op (REGION_PAINT / REGION_CLEAR, brush material 0..253) over the selected components — those
        holding one of `seeds` ((n, 3) voxels), touching `regions` (one Region or a list) and of min_voxels..max_voxels voxels,
        or (invert) all others; rebuilds the bound tree in place and returns the canonical tree's cell count.  seeds / regions
        None: no such filter; an empty list: a filter that matches nothing (so a click on nothing edits nothing)."""
        sel = self._select(connectivity, match, min_voxels, max_voxels, invert)
        s, ns = _seeds(seeds)
        arr, k = _touch_regions(regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_connected(self.h, int(op), ctypes.byref(sel), s.ctypes.data if ns else None, ns, arr, k,
                                                         int(material), ctypes.byref(n)), n)
        return int(n.value)

    def octree_extract_connected(self, seeds=None, regions=None, connectivity=6, match=MATCH_ANY, min_voxels=0, max_voxels=2**32 - 1,
                                 invert=False):
        """tdt_octree_extract_connected: the selected components' voxels, (n, 4) int32 {x, y, z, material + 1}, Morton-sorted;
        seeds / regions as octree_edit_connected.  One labelling: the output is sized by the tree's voxel count (a walk), an upper
        bound of the selection."""
        sel = self._select(connectivity, match, min_voxels, max_voxels, invert)
        s, ns = _seeds(seeds)
        arr, k = _touch_regions(regions)
        sp = s.ctypes.data if ns else None
        out = np.empty((self._voxel_count(), 4), np.int32)
        n = ctypes.c_size_t(0)
        self.check(lib().tdt_octree_extract_connected(self.h, ctypes.byref(sel), sp, ns, arr, k, out.ctypes.data if len(out) else None,
                                                      len(out), ctypes.byref(n)))
        return out[: n.value].copy()

    @staticmethod
    def _morph(op, radius, connectivity, material, border):
        """struct tdt_morph (material None: inherit); every field must fit an int32 (ctypes would wrap it silently) and a bool is
        not a number here.  The ranges themselves are the library's to check."""
        material = -1 if material is None else material
        for name, v in (("op", op), ("radius", radius), ("connectivity", connectivity), ("material", material), ("border", border)):
            if isinstance(v, bool) and name != "border":
                raise ValueError(f"{name} must be an integer, not {v!r}")
            if int(v) != v or not -2**31 <= int(v) <= 2**31 - 1:
                raise ValueError(f"{name} must be an int32, not {v!r}")
        return Morph(int(op), int(connectivity), int(radius), int(material), int(border), 0)

    def octree_morph(self, op, radius=1, connectivity=6, material=None, border=0, regions=None):
        """tdt_octree_morph: op (MORPH_*) of `radius` steps with the 6- or 26-neighbourhood on the bound tree, rebuilt in place;
        new voxels inherit their material (None) or get `material` 0..253; border 1 treats the outside of the grid as solid;
        regions (one Region or a list): a mask outside of which nothing changes (None: no mask; an empty list: an empty mask, so
        nothing changes).  Returns the canonical tree's cell count."""
        m = self._morph(op, radius, connectivity, material, border)
        arr, k = _touch_regions(regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_morph(self.h, ctypes.byref(m), arr, k, ctypes.byref(n)), n)
        return int(n.value)

    def octree_extract_morph(self, op, radius=1, connectivity=6, material=None, border=0, regions=None):
        """tdt_octree_extract_morph: what octree_morph would leave, as an (n, 4) int32 list {x, y, z, material + 1}, Morton-sorted;
        the tree is untouched.  MORPH_SHELL with radius 1: the surface voxels.  The result's size is known only once it exists
        (a DILATE grows the list), so this counts first and fills second: two runs of the steps."""
        m = self._morph(op, radius, connectivity, material, border)
        arr, k = _touch_regions(regions)
        return self._list(lib().tdt_octree_extract_morph, ctypes.byref(m), arr, k)

    def voxelize_triangles(self, vertices, triangles, depth, materials=None, material=0):
        """tdt_voxelize_triangles: the voxels of the grid [0, 2^depth)^3 the closed triangles touch, as an (n, 4) int32 list
        {x, y, z, material + 1}, Morton-sorted; vertices (n, 3) int32 fixed point (64 units per voxel; host.mesh_quantize),
        triangles (m, 3) indices, materials None or (m,) material + 1 per triangle (the highest covering triangle wins).
        Needs no bound tree.  Counts first, fills second: two rasterisations."""
        mesh, keep = _mesh(vertices, triangles, materials, material)
        out = self._list(lib().tdt_voxelize_triangles, ctypes.byref(mesh), int(depth))
        del keep
        return out

    def octree_edit_triangles(self, op, vertices, triangles, materials=None, material=0):
        """tdt_octree_edit_triangles: octree_edit_voxels(op, voxelize_triangles(..., max_depth of slot 7)) without the list
        leaving the device; returns the canonical tree's cell count."""
        mesh, keep = _mesh(vertices, triangles, materials, material)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_triangles(self.h, int(op), ctypes.byref(mesh), ctypes.byref(n)), n)
        del keep
        return int(n.value)

    def voxelize_stroke(self, points, radius, depth, segments=None, materials=None, material=0, shape=SHAPE_SPHERE):
        """tdt_voxelize_stroke: the voxels of the grid [0, 2^depth)^3 within `radius` of the stroke's segments — Euclidean for
        SHAPE_SPHERE, Chebyshev for SHAPE_BOX — as an (n, 4) int32 list {x, y, z, material + 1}, Morton-sorted; points (n, 3)
        voxel coordinates on or off the grid, segments None (the polyline of the points; one point: a dab) or (m, 2) point
        indices, materials None or material + 1 per segment (the highest covering segment wins).  Needs no bound tree.  Counts
        first, fills second: two sweeps."""
        stroke, keep = _stroke(points, radius, segments, materials, material, shape, depth=depth)
        out = self._list(lib().tdt_voxelize_stroke, ctypes.byref(stroke), int(depth))
        del keep
        return out

    def octree_edit_stroke(self, op, points, radius, segments=None, materials=None, material=0, shape=SHAPE_SPHERE):
        """tdt_octree_edit_stroke: octree_edit_voxels(op, voxelize_stroke(..., max_depth of slot 7)) without the list leaving the
        device; returns the canonical tree's cell count."""
        stroke, keep = _stroke(points, radius, segments, materials, material, shape, op=op)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_stroke(self.h, int(op), ctypes.byref(stroke), ctypes.byref(n)), n)
        del keep
        return int(n.value)

    def octree_extract_stroke(self, points, radius, segments=None, shape=SHAPE_SPHERE):
        """tdt_octree_extract_stroke: the bound tree's voxels the stroke covers, with the tree's materials, (n, 4) int32,
        Morton-sorted: the undo record of a CLEAR or PAINT stroke (octree_edit_voxels(REGION_SET, it) puts them back)."""
        stroke, keep = _stroke(points, radius, segments, None, 0, shape)
        out = self._list(lib().tdt_octree_extract_stroke, ctypes.byref(stroke))
        del keep
        return out

    @staticmethod
    def _fill(connectivity, material):
        """struct tdt_fill (material None: inherit); both fields must fit an int32 (ctypes would wrap them silently) and a bool is
        not a number here.  The ranges themselves are the library's to check."""
        material = -1 if material is None else material
        for name, v in (("connectivity", connectivity), ("material", material)):
            if isinstance(v, bool):
                raise ValueError(f"{name} must be an integer, not {v!r}")
            if int(v) != v or not -2**31 <= int(v) <= 2**31 - 1:
                raise ValueError(f"{name} must be an int32, not {v!r}")
        return Fill(int(connectivity), int(material))

    def octree_extract_enclosed(self, connectivity=6, material=None, regions=None):
        """tdt_octree_extract_enclosed: the empty voxels of the bound tree that no path of empty 6- / 26-neighbours connects to a
        face of the grid, as an (n, 4) int32 list {x, y, z, material + 1}, Morton-sorted; they inherit the material of the wall
        at their -x side (None) or get `material` 0..253; regions (one Region or a list) limit what is reported (None: no mask;
        an empty list: an empty mask).  The tree is untouched.  Counts first, fills second: two floods."""
        f = self._fill(connectivity, material)
        arr, k = _touch_regions(regions)
        return self._list(lib().tdt_octree_extract_enclosed, ctypes.byref(f), arr, k)

    def octree_fill_enclosed(self, connectivity=6, material=None, regions=None):
        """tdt_octree_fill_enclosed: octree_edit_voxels(REGION_FILL, octree_extract_enclosed(...)) without the list leaving the
        device; rebuilds the bound tree in place and returns the canonical tree's cell count."""
        f = self._fill(connectivity, material)
        arr, k = _touch_regions(regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_fill_enclosed(self.h, ctypes.byref(f), arr, k, ctypes.byref(n)), n)
        return int(n.value)

    def voxelize_triangles_solid(self, vertices, triangles, depth, materials=None, material=0, connectivity=6, fill_material=None):
        """tdt_voxelize_triangles_solid: voxelize_triangles(...) plus the space its surface encloses (connectivity of the empty
        voxels 6 / 26; fill_material None: inherit the surface's material along -x, or 0..253), (n, 4) int32, Morton-sorted.
        Needs no bound tree.  Counts first, fills second."""
        mesh, keep = _mesh(vertices, triangles, materials, material)
        f = self._fill(connectivity, fill_material)
        out = self._list(lib().tdt_voxelize_triangles_solid, ctypes.byref(mesh), int(depth), ctypes.byref(f))
        del keep
        return out

    def octree_edit_triangles_solid(self, op, vertices, triangles, materials=None, material=0, connectivity=6, fill_material=None):
        """tdt_octree_edit_triangles_solid: octree_edit_voxels(op, voxelize_triangles_solid(..., max_depth of slot 7)) without the
        list leaving the device; returns the canonical tree's cell count."""
        mesh, keep = _mesh(vertices, triangles, materials, material)
        f = self._fill(connectivity, fill_material)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_triangles_solid(self.h, int(op), ctypes.byref(mesh), ctypes.byref(f), ctypes.byref(n)), n)
        del keep
        return int(n.value)

    @staticmethod
    def _surface(merge, by_material):
        """struct tdt_surface; both fields must fit an int32 (ctypes would wrap them silently); True / False are 1 / 0.  The ranges
        themselves are the library's to check."""
        for name, v in (("merge", merge), ("by_material", by_material)):
            if int(v) != v or not -2**31 <= int(v) <= 2**31 - 1:
                raise ValueError(f"{name} must be an int32, not {v!r}")
        return Surface(int(merge), int(by_material))

    def octree_extract_surface(self, merge=True, by_material=True, regions=None):
        """tdt_octree_extract_surface: the exposed faces of the bound tree's voxels as an (n, 8) int32 array of tdt_quad rows {face,
        material, origin[3], size[2], pad}, ordered by face, w, u0, v0; merge: runs, then stacks of identical runs (False: one
        1 x 1 quad per face); by_material: faces carry material + 1 and merge within a material only (False: they carry 0);
        regions (one Region or a list) limit the voxels whose faces are reported (None: no mask; an empty list: an empty mask).
        The tree is untouched.  Counts first, fills second: two extractions."""
        s = self._surface(merge, by_material)
        arr, k = _touch_regions(regions)
        return self._list(lib().tdt_octree_extract_surface, ctypes.byref(s), arr, k, width=8)

    def octree_face_regions(self, connectivity=4, match=MATCH_MATERIAL, regions=None, capacity=4096):
        """tdt_octree_face_regions: (faces, labels, table) of the bound tree's exposed faces — faces the (n, 8) int32 tdt_quad rows
        of octree_extract_surface(merge=False) under the same mask, labels (n,) uint32 the face region of each, table a
        FACE_REGION_DTYPE array numbered in the order of each region's first face.  connectivity 4 / 8 inside a plane; match
        MATCH_*; regions confine the regions (None: no mask; an empty list: an empty mask).  Labels once where it can, as
        octree_components does: the arrays are sized by `capacity`, and only a tree with more faces or regions is labelled a
        second time, into arrays of the sizes the first call reported."""
        _faces(np.zeros((0, 4), np.int32), 0, connectivity, match)
        arr, k = _touch_regions(regions)
        nf, nr = ctypes.c_size_t(0), ctypes.c_size_t(0)
        cap = max(int(capacity), 1)
        faces, labels, table = np.zeros((cap, 8), np.int32), np.zeros(cap, np.uint32), np.zeros(cap, FACE_REGION_DTYPE)

        def run():
            return lib().tdt_octree_face_regions(self.h, int(connectivity), int(match), arr, k, faces.ctypes.data, labels.ctypes.data, len(labels),
                                                 ctypes.byref(nf), table.ctypes.data, len(table), ctypes.byref(nr))

        rc = run()
        if rc == ERR_INVALID_VALUE and (nf.value > len(labels) or nr.value > len(table)):
            faces, labels = np.zeros((max(nf.value, 1), 8), np.int32), np.zeros(max(nf.value, 1), np.uint32)
            table = np.zeros(max(nr.value, 1), FACE_REGION_DTYPE)
            rc = run()
        self.check(rc)
        return faces[: nf.value].copy(), labels[: nf.value].copy(), table[: nr.value].copy()

    def octree_extract_faces(self, seeds, distance, what=FACES_COLUMNS, connectivity=4, match=MATCH_MATERIAL, block=False, material=-1,
                             regions=None):
        """tdt_octree_extract_faces: for the face regions under `seeds` ((n, 4) int32 {x, y, z, f}; host.pick_face makes one from a
        pick) swept by the signed `distance`, FACES_COLUMNS: the column list {x, y, z, material + 1} (the preview, what
        Texture.overlay takes); FACES_TREE: the bound tree's voxels the columns cover, with the tree's materials (the undo record
        before a push, a paint or a SET pull).  (n, 4) int32, Morton-sorted.  Counts first, fills second: two sweeps."""
        f, s = _faces(seeds, distance, connectivity, match, block, material, what=what)
        arr, k = _touch_regions(regions)
        return self._list(lib().tdt_octree_extract_faces, ctypes.byref(f), s.ctypes.data if len(s) else None, len(s), arr, k, int(what))

    def octree_edit_faces(self, op, seeds, distance, connectivity=4, match=MATCH_MATERIAL, block=False, material=-1, regions=None):
        """tdt_octree_edit_faces: octree_edit_voxels(op, octree_extract_faces(..., FACES_COLUMNS)) without the list leaving the
        device: pull (REGION_FILL / REGION_SET, distance > 0), push (REGION_CLEAR, distance < 0), paint a face (REGION_PAINT,
        distance -1); returns the canonical tree's cell count.  No seed or distance 0 installs the compacted tree."""
        f, s = _faces(seeds, distance, connectivity, match, block, material, op=op)
        arr, k = _touch_regions(regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_faces(self.h, int(op), ctypes.byref(f), s.ctypes.data if len(s) else None, len(s), arr, k,
                                                     ctypes.byref(n)), n)
        return int(n.value)

    def debug_faces_premerge(self, on):
        """tdt_debug_faces_premerge: the face labelling's hook stage with (True, the default) or without the in-wave pre-merge of
        runs; both label alike.  Measurement only."""
        self.check(lib().tdt_debug_faces_premerge(self.h, 1 if on else 0))

    @staticmethod
    def _int32(name, v, allow_bool=False):
        """v as an int that fits an int32 (ctypes would wrap it silently); a float with a fraction or a bool is not a number here."""
        if isinstance(v, bool) and not allow_bool:
            raise ValueError(f"{name} must be an integer, not {v!r}")
        if int(v) != v or not -2**31 <= int(v) <= 2**31 - 1:
            raise ValueError(f"{name} must be an int32, not {v!r}")
        return int(v)

    @classmethod
    def _box3(cls, lo, hi):
        """The corners of an inclusive box as two checked int32[3] arrays."""
        box3 = []
        for name, c in (("lo", lo), ("hi", hi)):
            c = list(c)
            if len(c) != 3:
                raise ValueError(f"{name} must hold three coordinates")
            box3.append((ctypes.c_int32 * 3)(*[cls._int32(name, v) for v in c]))
        return box3

    @classmethod
    def _round(cls, op, radius2, material, border):
        """struct tdt_round (material None: inherit).  The ranges themselves are the library's to check."""
        material = -1 if material is None else material
        return Round(cls._int32("op", op), cls._int32("radius2", radius2), cls._int32("material", material),
                     cls._int32("border", border, allow_bool=True))

    def octree_morph_round(self, op, radius2, material=None, border=0, regions=None):
        """tdt_octree_morph_round: op (MORPH_*) with the Euclidean ball of squared radius `radius2` (1..4096) on the bound tree,
        rebuilt in place; new voxels inherit the material of their nearest voxel (None) or get `material` 0..253; border 1 treats
        the outside of the grid as solid; regions: a mask as in octree_morph.  Returns the canonical tree's cell count."""
        r = self._round(op, radius2, material, border)
        arr, k = _touch_regions(regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_morph_round(self.h, ctypes.byref(r), arr, k, ctypes.byref(n)), n)
        return int(n.value)

    def octree_extract_morph_round(self, op, radius2, material=None, border=0, regions=None):
        """tdt_octree_extract_morph_round: what octree_morph_round would leave, as an (n, 4) int32 list {x, y, z, material + 1},
        Morton-sorted; the tree is untouched.  Counts first, fills second: two transforms."""
        r = self._round(op, radius2, material, border)
        arr, k = _touch_regions(regions)
        return self._list(lib().tdt_octree_extract_morph_round, ctypes.byref(r), arr, k)

    def octree_distance_field(self, lo, hi, max_d2, border=0, nearest=False):
        """tdt_octree_distance_field: the signed squared Euclidean distance over the inclusive box lo..hi as an (ez, ey, ex) int32
        array: +d2 to the nearest voxel for an empty voxel, -d2 to the nearest empty point for an occupied one (border 0: the
        points outside the grid count), magnitudes above max_d2 (1..4096) reported as max_d2 + 1.  nearest: also an (ez, ey, ex,
        3) array of the nearest voxel {x, y, z} (an occupied voxel: itself; none within max_d2: -1).  The tree is untouched."""
        box3 = self._box3(lo, hi)
        max_d2, border = self._int32("max_d2", max_d2), self._int32("border", border, allow_bool=True)
        n = ctypes.c_size_t(0)
        self.check(lib().tdt_octree_distance_field(self.h, box3[0], box3[1], max_d2, border, None, None, 0, ctypes.byref(n)))
        ex, ey, ez = (int(box3[1][a]) - int(box3[0][a]) + 1 for a in range(3))
        field = np.zeros((ez, ey, ex), np.int32)
        near = np.zeros((ez, ey, ex, 3), np.int32) if nearest else None
        assert field.size == n.value
        self.check(lib().tdt_octree_distance_field(self.h, box3[0], box3[1], max_d2, border, field.ctypes.data,
                                                   near.ctypes.data if nearest else None, field.size, ctypes.byref(n)))
        return (field, near) if nearest else field

    @classmethod
    def _smooth(cls, radius2, iterations, threshold, mode, material, border):
        """struct tdt_smooth (threshold None: majority; material None: inherit).  The ranges themselves are the library's to check."""
        threshold = 0 if threshold is None else threshold
        material = -1 if material is None else material
        return Smooth(cls._int32("radius2", radius2), cls._int32("iterations", iterations), cls._int32("threshold", threshold),
                      cls._int32("mode", mode), cls._int32("material", material), cls._int32("border", border, allow_bool=True))

    def octree_smooth(self, radius2, iterations=1, threshold=None, mode=SMOOTH_BOTH, material=None, border=0, regions=()):
        """tdt_octree_smooth: `iterations` (1..16) steps of the ball-density threshold filter on the bound tree, rebuilt in place.
        A step keeps (SMOOTH_BOTH), adds (SMOOTH_ADD) or removes (SMOOTH_REMOVE) by the test "the ball of squared radius `radius2`
        (1..225) around the voxel holds more than half of its support" (threshold None) or "at least threshold / 65536 of it"
        (1..65536); new voxels inherit the material of their nearest voxel (None) or get `material` 0..253; border 1 leaves the
        outside of the grid out of the vote; regions: one Region or a sequence limits what a step may change (none, as the C
        call's n_regions = 0: no mask).  Returns the canonical tree's cell count."""
        s = self._smooth(radius2, iterations, threshold, mode, material, border)
        arr, k = _regions(() if regions is None else regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_smooth(self.h, ctypes.byref(s), arr, k, ctypes.byref(n)), n)
        return int(n.value)

    def octree_extract_smooth(self, radius2, iterations=1, threshold=None, mode=SMOOTH_BOTH, material=None, border=0, regions=()):
        """tdt_octree_extract_smooth: what octree_smooth would leave, as an (n, 4) int32 list {x, y, z, material + 1},
        Morton-sorted; the tree is untouched.  Counts first, fills second: the filter runs twice."""
        s = self._smooth(radius2, iterations, threshold, mode, material, border)
        arr, k = _regions(() if regions is None else regions)
        return self._list(lib().tdt_octree_extract_smooth, ctypes.byref(s), arr, k)

    def octree_density_field(self, lo, hi, radius2, support=False):
        """tdt_octree_density_field: how many voxels of the bound tree the ball of squared radius `radius2` (1..225) around each
        voxel of the inclusive box lo..hi holds, as an (ez, ey, ex) int32 array.  support: also an array of the same shape with the
        number of ball points inside the grid.  The tree is untouched."""
        box3 = self._box3(lo, hi)
        radius2 = self._int32("radius2", radius2)
        n = ctypes.c_size_t(0)
        self.check(lib().tdt_octree_density_field(self.h, box3[0], box3[1], radius2, None, None, 0, ctypes.byref(n)))
        ex, ey, ez = (int(box3[1][a]) - int(box3[0][a]) + 1 for a in range(3))
        density = np.zeros((ez, ey, ex), np.int32)
        sup = np.zeros((ez, ey, ex), np.int32) if support else None
        assert density.size == n.value
        self.check(lib().tdt_octree_density_field(self.h, box3[0], box3[1], radius2, density.ctypes.data,
                                                  sup.ctypes.data if support else None, density.size, ctypes.byref(n)))
        return (density, sup) if support else density

    @classmethod
    def _xform(cls, xf):
        """A checked copy of an Xform, or one built from a dict / keywords-like mapping with the keys t, a, material (None: -1),
        dst_lo, dst_hi.  Every entry must be an integer that fits its field (ctypes would wrap it silently); a bool is not a number
        here.  The ranges themselves are the library's to check."""
        if isinstance(xf, Xform):
            get = lambda k, d: getattr(xf, k)                                # noqa: E731
        elif isinstance(xf, dict):
            get = lambda k, d: xf.get(k, d)                                  # noqa: E731
        else:
            raise ValueError(f"xf must be an rt.Xform or a dict, not {type(xf).__name__}")

        def ints(name, v, count, bits):
            v = list(v)
            if len(v) != count:
                raise ValueError(f"{name} must hold {count} entries")
            for e in v:
                if isinstance(e, (bool, np.bool_)) or int(e) != e or not -2 ** (bits - 1) <= int(e) <= 2 ** (bits - 1) - 1:
                    raise ValueError(f"{name} must hold int{bits} values, not {e!r}")
            return [int(e) for e in v]
        material = get("material", -1)
        out = Xform()
        out.t[:] = ints("t", get("t", (0, 0, 0)), 3, 64)
        out.a[:] = ints("a", get("a", (XFORM_ONE, 0, 0, 0, XFORM_ONE, 0, 0, 0, XFORM_ONE)), 9, 32)
        out.material = cls._int32("material", -1 if material is None else material)
        out.dst_lo[:] = ints("dst_lo", get("dst_lo", (0, 0, 0)), 3, 32)
        out.dst_hi[:] = ints("dst_hi", get("dst_hi", (2 ** 31 - 1,) * 3), 3, 32)
        out.pad[:] = ints("pad", get("pad", (0, 0)), 2, 32)
        return out

    def octree_transform(self, xf, op=REGION_SET, regions=None):
        """tdt_octree_transform: octree_edit_voxels(op, octree_extract_transform(xf, regions)) with the list taken from the tree
        before the edit and never leaving the device; xf an Xform (host.xform_*) or a dict of its fields.  The source voxels stay:
        a move clears them with octree_edit_region first.  Returns the canonical tree's cell count."""
        x = self._xform(xf)
        op = self._int32("op", op)
        arr, k = _touch_regions(regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_transform(self.h, ctypes.byref(x), op, arr, k, ctypes.byref(n)), n)
        return int(n.value)

    def octree_extract_transform(self, xf, regions=None):
        """tdt_octree_extract_transform: the transformed selection as an (n, 4) int32 list {x, y, z, material + 1}, Morton-sorted:
        every destination voxel p of the grid and of xf's dst box whose source voxel (a (2 p + 1) + t) >> 17 is a voxel of the
        tree inside `regions` (None: the whole tree; an empty list: nothing).  The tree is untouched.  Counts first, fills
        second: two resamplings."""
        x = self._xform(xf)
        arr, k = _touch_regions(regions)
        return self._list(lib().tdt_octree_extract_transform, ctypes.byref(x), arr, k)

    def xform_bricks(self):
        """tdt_debug_xform_bricks: (bricks of the last transform's destination domain, bricks its count and emit passes ran on)."""
        out = (ctypes.c_uint32 * 2)()
        self.check(lib().tdt_debug_xform_bricks(self.h, out))
        return int(out[0]), int(out[1])

    @classmethod
    def _geodesic(cls, medium, steps, max_cost, match, material, seeds):
        """(struct tdt_geodesic, the seed array, its count) of a geodesic call: steps three weights (STEPS_6, STEPS_26, CHAMFER_345
        or any other), match / material None = -1.  Every entry must fit an int32 (ctypes would wrap it silently); the ranges
        themselves are the library's to check.  Seeds: an (n, 3) array; none is a valid call with an empty result."""
        steps = list(steps)
        if len(steps) != 3:
            raise ValueError("steps must hold three weights")
        g = Geodesic(cls._int32("medium", medium), cls._int32("match", -1 if match is None else match),
                     (ctypes.c_int32 * 3)(*[cls._int32("steps", v) for v in steps]), cls._int32("max_cost", max_cost),
                     cls._int32("material", -1 if material is None else material), 0)
        s = np.ascontiguousarray(_exact_ints(np.asarray(seeds).reshape(-1, 3) if len(seeds) else np.zeros((0, 3), np.int32), np.int32, "seeds"))
        return g, s, len(s)

    def octree_geodesic_field(self, seeds, lo, hi, medium=MEDIUM_SOLID, steps=STEPS_6, max_cost=1 << 30, match=None, regions=None):
        """tdt_octree_geodesic_field: the geodesic distance g from the seeds ((n, 3) voxel coordinates) through the medium
        (MEDIUM_SOLID: the tree's voxels, of LEAF value `match` only when given; MEDIUM_EMPTY: the empty voxels), a step across a
        face / an edge / a corner costing steps[0..2] (0: no such step), over the inclusive box lo..hi as an (ez, ey, ex) int32
        array; -1 where a voxel is not in the medium, unreachable or beyond max_cost.  regions (one Region or a list) confine the
        PATHS (None: no mask; an empty list: an empty mask, so nothing is reached).  The tree is untouched."""
        g, s, k = self._geodesic(medium, steps, max_cost, match, None, seeds)
        arr, kr = _touch_regions(regions)
        box3 = self._box3(lo, hi)
        n = ctypes.c_size_t(0)
        sp = s.ctypes.data if k else None
        self.check(lib().tdt_octree_geodesic_field(self.h, ctypes.byref(g), sp, k, arr, kr, box3[0], box3[1], None, 0, ctypes.byref(n)))
        ex, ey, ez = (int(box3[1][a]) - int(box3[0][a]) + 1 for a in range(3))
        field = np.zeros((ez, ey, ex), np.int32)
        assert field.size == n.value
        self.check(lib().tdt_octree_geodesic_field(self.h, ctypes.byref(g), sp, k, arr, kr, box3[0], box3[1], field.ctypes.data, field.size,
                                                   ctypes.byref(n)))
        return field

    def octree_extract_geodesic(self, seeds, medium=MEDIUM_SOLID, steps=STEPS_6, max_cost=1 << 30, match=None, material=None, regions=None):
        """tdt_octree_extract_geodesic: the reach set { g <= max_cost } of octree_geodesic_field's distance as an (n, 4) int32 list
        {x, y, z, material + 1}, Morton-sorted; material None: the voxel's own (MEDIUM_SOLID only), or 0..253.  The tree is
        untouched.  Counts first, fills second: two relaxations."""
        g, s, k = self._geodesic(medium, steps, max_cost, match, material, seeds)
        arr, kr = _touch_regions(regions)
        sp = s.ctypes.data if k else None
        return self._list(lib().tdt_octree_extract_geodesic, ctypes.byref(g), sp, k, arr, kr)

    def octree_edit_geodesic(self, op, seeds, medium=MEDIUM_SOLID, steps=STEPS_6, max_cost=1 << 30, match=None, material=None, regions=None):
        """tdt_octree_edit_geodesic: octree_edit_voxels(op, octree_extract_geodesic(...)) with the list taken from the tree before
        the edit and never leaving the device; returns the canonical tree's cell count."""
        g, s, k = self._geodesic(medium, steps, max_cost, match, material, seeds)
        op = self._int32("op", op)
        arr, kr = _touch_regions(regions)
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_geodesic(self.h, op, ctypes.byref(g), s.ctypes.data if k else None, k, arr, kr, ctypes.byref(n)), n)
        return int(n.value)

    def octree_geodesic_path(self, seeds, goal, medium=MEDIUM_SOLID, steps=STEPS_6, max_cost=1 << 30, match=None, regions=None):
        """tdt_octree_geodesic_path: (the canonical shortest path from `goal` back to the seed it reaches as an (n, 3) int32 array,
        path[0] = goal; g(goal)).  A goal outside the reach set: (an empty array, -1)."""
        g, s, k = self._geodesic(medium, steps, max_cost, match, None, seeds)
        arr, kr = _touch_regions(regions)
        goal = list(goal)
        if len(goal) != 3:
            raise ValueError("goal must hold three coordinates")
        q = (ctypes.c_int32 * 3)(*[self._int32("goal", v) for v in goal])
        cost = ctypes.c_int32(-1)
        out = self._list(lib().tdt_octree_geodesic_path, ctypes.byref(g), s.ctypes.data if k else None, k, arr, kr, q, width=3,
                         tail=(ctypes.byref(cost),))
        return out, int(cost.value)

    def geodesic_passes(self):
        """tdt_debug_geodesic_passes: the relaxation passes of the last geodesic call that changed the volume."""
        return int(lib().tdt_debug_geodesic_passes(self.h))

    def reproject_counts(self):
        """tdt_debug_reproject_counts: (keyed, found, rejected by key or sample count, rejected behind or off-screen) of the last
        Texture.reproject (blocks)."""
        c = (ctypes.c_uint64 * 4)()
        self.check(lib().tdt_debug_reproject_counts(self.h, c))
        return tuple(int(v) for v in c)

    def upsample_counts(self):
        """tdt_debug_upsample_counts: (pixels, validated bilinear, ring, holes) of the last Texture.upsample (blocks)."""
        c = (ctypes.c_uint64 * 4)()
        self.check(lib().tdt_debug_upsample_counts(self.h, c))
        return tuple(int(v) for v in c)

    def adapt_counts(self):
        """tdt_debug_adapt_counts: (live before, stopped by the tolerance, stopped by the cap, still live) of the last Texture.adapt
        (blocks)."""
        c = (ctypes.c_uint64 * 4)()
        self.check(lib().tdt_debug_adapt_counts(self.h, c))
        return tuple(int(v) for v in c)

    def overlay_counts(self):
        """tdt_debug_overlay_counts: (pixels, pixels with a voxel, member pixels, edge pixels) of the last Texture.overlay (blocks)."""
        c = (ctypes.c_uint64 * 4)()
        self.check(lib().tdt_debug_overlay_counts(self.h, c))
        return tuple(int(v) for v in c)

    def octree_extract_screen(self, view, rect=None, polygon=None, mask=None, window=False, material=None, min_distance=0.0,
                              max_distance=float("inf")):
        """tdt_octree_extract_screen: through-selection.  Every voxel of the bound tree whose centre (window: all eight of whose
        corners) projects, in `view` (a VIEW: ComputeShader.view()), into the screen shape — exactly one of rect = (x0, y0, x1, y1)
        inclusive, polygon = 3..256 integer vertices (even-odd rule at the pixel centre) and mask = a Texture of the view's size
        (inside where its red channel is > 0) — hidden or not, filtered by material (None: any) and by its centre's distance from
        the view's origin: (n, 4) int32 {x, y, z, material + 1}, Morton-sorted.  One walk: the output is sized by the tree's voxel
        count, an upper bound of the selection.  Blocks."""
        if not isinstance(view, VIEW):
            raise ValueError("view is a VIEW (ComputeShader.view())")
        sel, pts, mask = _screen_select(rect, polygon, mask, window, material, min_distance, max_distance)
        out = np.empty((self._voxel_count(), 4), np.int32)
        n = ctypes.c_size_t(0)
        self.check(lib().tdt_octree_extract_screen(self.h, ctypes.byref(view), ctypes.byref(sel), pts.ctypes.data if pts is not None else None,
                                                   len(pts) if pts is not None else 0, mask.h if mask is not None else None,
                                                   out.ctypes.data if len(out) else None, len(out), ctypes.byref(n)))
        return out[: n.value].copy()

    def octree_edit_screen(self, op, view, rect=None, polygon=None, mask=None, window=False, material=None, min_distance=0.0,
                           max_distance=float("inf"), paint_material=0):
        """tdt_octree_edit_screen: op REGION_PAINT (with paint_material 0..253) or REGION_CLEAR over what octree_extract_screen
        would return for the same arguments; the list never leaves the device.  Rebuilds the bound tree in place on every replica
        (a mask: single-device contexts only) and returns the canonical tree's cell count."""
        if not isinstance(view, VIEW):
            raise ValueError("view is a VIEW (ComputeShader.view())")
        sel, pts, mask = _screen_select(rect, polygon, mask, window, material, min_distance, max_distance)
        if not _is_int(paint_material) or not 0 <= paint_material <= 253:
            raise ValueError("paint_material must be an int 0..253")
        n = ctypes.c_uint32(0)
        self._check_edit(lib().tdt_octree_edit_screen(self.h, int(op), ctypes.byref(view), ctypes.byref(sel),
                                                      pts.ctypes.data if pts is not None else None, len(pts) if pts is not None else 0,
                                                      mask.h if mask is not None else None, int(paint_material), ctypes.byref(n)), n)
        return int(n.value)

    def screen_counts(self):
        """tdt_debug_screen_counts: (voxels of the tree, those whose tested points are all in front and on screen, of those the
        voxels inside the shape, voxels selected after the filters) of the last octree_extract_screen / octree_edit_screen (blocks)."""
        c = (ctypes.c_uint64 * 4)()
        self.check(lib().tdt_debug_screen_counts(self.h, c))
        return tuple(int(v) for v in c)

    def fill_passes(self):
        """tdt_debug_fill_passes: the flood passes of the last enclosed-space call that changed the volume."""
        return int(lib().tdt_debug_fill_passes(self.h))

    def bind_buffer_base(self, target, slot, vbo):
        """gl::BindBufferBase(target, slot, vbo.id()) — main.rs:352,383,408,430,448; octree.rs:67,98,115,144."""
        self.check(lib().tdt_bind_buffer_base(self.h, target, slot, vbo.h if vbo is not None else None))

    def selftest(self, which):
        """Mismatches of the short rcp (0) / sqrt (1) / rsq (2) forms vs IEEE over all 2^32 inputs; the other modes: include/tdt_rt.h
        (17: the whole-depth table of the bound cells buffer, every position; 18: its plane form, planes through the offsets vs arithmetic;
        19: the lanes in a band served from the table, every float of every band; its outcome counts: selftest_band_counts)."""
        n = ctypes.c_uint64(0)
        self.check(lib().tdt_selftest(self.h, which, ctypes.byref(n)))
        return n.value

    def selftest_band_counts(self):
        """After selftest(19): lanes resolved to position n, to n - 2^j, and left to the level walk."""
        c = (ctypes.c_uint64 * 32)()
        self.check(lib().tdt_debug_counters(self.h, c))
        return {"to_n": int(c[1]), "to_lower": int(c[2]), "to_walk": int(c[3])}

    def last_variant(self):
        """The build of the trace kernel the last trace launch ran: dict(form, depth, resident, full, brick, unit) and its launch
        geometry (block = threads per block, per_cu = blocks that share a CU); depth 0 = general kernel."""
        v, g = (ctypes.c_int * 6)(), (ctypes.c_int * 2)()
        self.check(lib().tdt_debug_last_variant(self.h, v))
        self.check(lib().tdt_debug_last_geometry(self.h, g))
        return dict(zip(("form", "depth", "resident", "full", "brick", "unit", "block", "per_cu"), [int(x) for x in v] + [int(x) for x in g]))

    STAT_NAMES = ("trav_pass", "trav_lanes", "inside_lanes", "alive_lanes", "event_pass", "event_lanes", "hit_pass", "hit_lanes", "lamb_pass", "lamb_lanes",
                  "metal_pass", "metal_lanes", "diel_pass", "diel_lanes", "end_pass", "end_lanes", "pixel_end_pass", "pixel_end_lanes", "fetch_pass", "fetch_lanes",
                  "primary_pass", "primary_lanes", "newray_pass", "newray_lanes", "gate_wait_lanes", "drained_trav_pass", "drained_event_pass", "loop_pass",
                  "wave_ticks", "waves", "t_first", "t_last", "fallback_pass", "fallback_lanes", "band_pass", "band_lanes", "resolved_lanes")

    def stats(self, reset=True):
        """Pass / lane statistics of the product trace kernels since the last reset (a -DTDT_STATS build of the library only)."""
        rows = len(self.STAT_NAMES)
        n = rows + 1 + 8192
        v = (ctypes.c_uint64 * n)()
        self.check(lib().tdt_debug_stats(self.h, v, n, 1 if reset else 0))
        d = dict(zip(self.STAT_NAMES, [int(x) for x in v[:rows]]))
        d["t_queue_dry"] = int(v[rows])
        d["wave_ends"] = [int(x) for x in v[rows + 1:rows + 1 + min(d["waves"], 8192)]]
        return d

    def selftest_index(self, cell_count, inv_cell_count, n_cells, shift=0):
        """(mismatches, shape_ok) of the per-cell x-index thresholds vs the literal formula: every f in [0,1) x every cell < n_cells."""
        n, ok = ctypes.c_uint64(0), ctypes.c_int(0)
        self.check(lib().tdt_selftest_index(self.h, int(cell_count), float(inv_cell_count), int(n_cells), int(shift), ctypes.byref(n), ctypes.byref(ok)))
        return n.value, bool(ok.value)

    def close(self):
        if self.h:
            lib().tdt_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class VertexBufferObject:
    """VertexBufferObject::new::<T>(Vec<T>, ..): glGenBuffers + glBufferData (copies) — vbo.rs:32-55."""

    def __init__(self, ctx, data):
        a = np.ascontiguousarray(data)
        h = ctypes.c_void_p()
        ctx.check(lib().tdt_buffer_create(ctx.h, a.ctypes.data if a.size else None, a.nbytes, ctypes.byref(h)))
        self.ctx, self.h, self.nbytes = ctx, h, a.nbytes

    @classmethod
    def _adopt(cls, ctx, h, nbytes):
        b = cls.__new__(cls)
        b.ctx, b.h, b.nbytes = ctx, h, nbytes
        return b

    def sub_data(self, offset, data):
        a = np.ascontiguousarray(data)
        self.ctx.check(lib().tdt_buffer_sub_data(self.h, offset, a.nbytes, a.ctypes.data))

    def read(self, dtype=np.uint32):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        self.ctx.check(lib().tdt_buffer_read(self.h, 0, out.nbytes, out.ctypes.data))
        return out


class Texture:
    """Texture::new_2d(TEXTURE0, 0, RGBA32F, RGBA, w, h) + BindImageTexture(unit 0) — texture.rs:47-75."""

    def __init__(self, ctx, h, width, height):
        self.ctx, self.h, self._w, self._h = ctx, h, width, height

    @classmethod
    def new_2d(cls, ctx, width, height, bind=True):
        h = ctypes.c_void_p()
        ctx.check(lib().tdt_image_create_rgba32f(ctx.h, width, height, ctypes.byref(h)))
        t = cls(ctx, h, width, height)
        if bind:
            t.bind()
        return t

    @classmethod
    def wrap_device(cls, ctx, device_ptr, width, height, bind=True):
        h = ctypes.c_void_p()
        ctx.check(lib().tdt_image_wrap_device(ctx.h, ctypes.c_void_p(device_ptr), width, height, ctypes.byref(h)))
        t = cls(ctx, h, width, height)
        if bind:
            t.bind()
        return t

    def bind(self):
        self.ctx.check(lib().tdt_bind_image(self.ctx.h, 0, self.h))

    def width(self):
        return self._w

    def height(self):
        return self._h

    def depth(self):
        return 1

    def read(self):
        img = np.empty((self._h, self._w, 4), np.float32)
        self.ctx.check(lib().tdt_image_read(self.h, img.ctypes.data))
        return img

    def read_rgba8(self, top_down=True):
        """The frame as the reference's quad pass presents it (quad.frag:10, main.rs:582-600): (H, W, 4) uint8, converted on
        the GPU; top_down=True puts the top scan-line first (image-file order)."""
        img = np.empty((self._h, self._w, 4), np.uint8)
        self.ctx.check(lib().tdt_image_read_rgba8(self.h, 1 if top_down else 0, img.ctypes.data))
        return img

    def denoise(self, guide, passes):
        """tdt_image_denoise: `passes` (0..8) a-trous passes of step 1, 2, 4, .. over this image, in place, averaging only pixels
        whose texels of `guide` (a Texture of this size that ComputeShader.dispatch_guide filled) carry the same surface key
        (kind, material, plane); kind-0 pixels pass through.  Asynchronous."""
        self.ctx.check(lib().tdt_image_denoise(self.h, guide.h, int(passes), 0))

    def read_guide(self):
        """The texels of a guide image as an (H, W) array of GUIDE_TEXEL_DTYPE (kind, material, plane, t)."""
        return self.read().view(GUIDE_TEXEL_DTYPE).reshape(self._h, self._w)

    def clear(self):
        """tdt_image_clear: every byte of the image to zero (before accumulating a sample range that does not start at 0).  A
        multi-device context's image is refused: there the running sums live in the members' tile buffers."""
        self.ctx.check(lib().tdt_image_clear(self.h))

    def reproject(self, shader, sample, guide, spp, prev=None, max_samples=64.0, hist_out=None, mean_out=None):
        """tdt_image_reproject with this texture as `sums` (running sums of `spp` samples): hist_out receives the sums plus, where an
        earlier frame saw the same surface point, that frame's history; prev = (VIEW, guide Texture, history Texture) of the earlier
        frame or None for a first frame; `guide` is what shader.dispatch_guide(guide, sample) wrote under the current camera.
        mean_out (may be this texture) receives history rgb / history alpha.  Asynchronous."""
        if hist_out is None:
            raise ValueError("reproject needs a history texture to write (hist_out)")
        view, pg, ph = prev if prev is not None else (None, None, None)
        self.ctx.check(lib().tdt_image_reproject(shader.h, int(sample), guide.h, self.h, int(spp), ctypes.byref(view) if view is not None else None,
                                                 pg.h if pg is not None else None, ph.h if ph is not None else None, float(max_samples),
                                                 hist_out.h, mean_out.h if mean_out is not None else None, 0))

    def variance(self, guide, moments=None, min_frames=4.0):
        """tdt_image_variance: this image's alpha becomes the variance of the luminance of its rgb — 0 for kind-0 pixels, from the
        temporal moments (a Texture that reproject_moments wrote) where a pixel has at least min_frames frames behind it, from
        its 7x7 same-key neighbourhood elsewhere.  rgb is left as it is.  Asynchronous."""
        self.ctx.check(lib().tdt_image_variance(self.h, guide.h, moments.h if moments is not None else None, float(min_frames), 0))

    def denoise_variance(self, guide, passes, sigma, floor=0.0):
        """tdt_image_denoise_variance: denoise's passes with a second edge-stopping weight max(lim - d^2, 0) on the difference d of
        luminance, lim = sigma^2 * (the centre's 3x3 prefiltered variance, read from alpha) + floor; alpha carries the variance of
        the filtered pixel on.  Pixels of kind 0, and those whose lim is not positive and finite, are copied.  Asynchronous."""
        self.ctx.check(lib().tdt_image_denoise_variance(self.h, guide.h, int(passes), float(sigma), float(floor), 0))

    def reproject_moments(self, shader, sample, guide, spp, prev=None, max_samples=64.0, hist_out=None, moments_out=None, mean_out=None):
        """tdt_image_reproject_moments: reproject, and moments_out receives (sum of the frames' luminances, sum of their squares,
        frame count, 0) joined with the earlier frame's moments wherever its history was found; prev = (VIEW, guide Texture, history
        Texture, moments Texture) of the earlier frame or None for a first frame.  Asynchronous."""
        if hist_out is None or moments_out is None:
            raise ValueError("reproject_moments needs a history and a moments texture to write (hist_out, moments_out)")
        view, pg, ph, pm = prev if prev is not None else (None, None, None, None)
        self.ctx.check(lib().tdt_image_reproject_moments(shader.h, int(sample), guide.h, self.h, int(spp),
                                                         ctypes.byref(view) if view is not None else None, pg.h if pg is not None else None,
                                                         ph.h if ph is not None else None, pm.h if pm is not None else None, float(max_samples),
                                                         hist_out.h, moments_out.h, mean_out.h if mean_out is not None else None, 0))

    def upsample(self, dst_guide, src, src_guide):
        """tdt_image_upsample into this texture: `src` (sums traced at reduced resolution) spread over this image's pixels, each
        taking only texels whose key in `src_guide` equals its own in `dst_guide` (a Texture of this size; src_guide of src's):
        validated bilinear, else the mean of the same-key texels of the 4x4 ring, else the nearest texel.  Asynchronous."""
        self.ctx.check(lib().tdt_image_upsample(self.h, dst_guide.h, src.h, src_guide.h, 0))

    def adapt(self, guide, state_in, state_out, spp_count, tolerance, floor=0.0, min_samples=0, max_samples=1 << 24):
        """tdt_image_adapt with this texture as `sums`: after a batch of spp_count samples for the live pixels of state_in,
        state_out receives every live pixel's updated (L, m2, n, w) with w negated where the pixel stops — the error of its mean
        luminance is below tolerance * max(mean, floor), with a guide (may be None) in its whole same-key 3x3 neighbourhood, or it
        has max_samples.  state_out is the next ComputeShader.dispatch_accumulate_masked's mask.  Asynchronous."""
        a = Adapt(float(tolerance), float(floor), int(min_samples), int(max_samples))
        self.ctx.check(lib().tdt_image_adapt(self.h, guide.h if guide is not None else None, state_in.h, state_out.h, int(spp_count),
                                             ctypes.byref(a), 0))

    def adapt_mean(self, state):
        """tdt_image_adapt_mean: this texture's running sums become means, rgb / the sample count |w| of `state`, and alpha the
        variance of the mean luminance; pixels without samples are left alone.  Asynchronous."""
        self.ctx.check(lib().tdt_image_adapt_mean(self.h, state.h, 0))

    def read_voxel_ids(self):
        """The texels of a voxel-id image as an (H, W) array of VOXEL_ID_TEXEL_DTYPE (state, key, material, t: the bits of hit.t)."""
        return self.read().view(VOXEL_ID_TEXEL_DTYPE).reshape(self._h, self._w)

    def overlay(self, ids, voxels, fill, edge=None, edge_width=1, voxel_edges=False):
        """tdt_image_overlay over this texture, in place: the pixels whose voxel in `ids` (a Texture of this size that
        ComputeShader.dispatch_voxel_ids filled) is in `voxels` — an (n, 4) int32 list {x, y, z, m}, m ignored, any order — are
        blended with fill = (r, g, b, a), those within edge_width pixels of the selection's border (voxel_edges: of their
        voxel's) with edge (None: fill).  The passes are queued; `voxels` may be dropped on return."""
        style = _overlay(fill, edge, edge_width, voxel_edges)
        v = np.ascontiguousarray(np.asarray(voxels, np.int32).reshape(-1, 4))
        self.ctx.check(lib().tdt_image_overlay(self.h, ids.h, v.ctypes.data if len(v) else None, len(v), ctypes.byref(style)))

    def extract_voxels(self, rect=None):
        """tdt_image_extract_voxels of this voxel-id image: the distinct voxels visible inside rect = (x0, y0, x1, y1), inclusive
        and clipped to the image (None: all of it), as an (n, 4) int32 array {x, y, z, material + 1}, Morton-sorted: the brush of
        Context.octree_edit_voxels.  Blocks."""
        r = None
        if rect is not None:
            if len(rect) != 4:
                raise ValueError("extract_voxels: rect is (x0, y0, x1, y1)")
            r = (ctypes.c_int32 * 4)(*[int(v) for v in rect])
        n = ctypes.c_size_t(0)
        self.ctx.check(lib().tdt_image_extract_voxels(self.h, r, None, 0, ctypes.byref(n)))
        out = np.zeros((n.value, 4), np.int32)
        if n.value:
            self.ctx.check(lib().tdt_image_extract_voxels(self.h, r, out.ctypes.data, n.value, ctypes.byref(n)))
        return out

    def device_ptr(self):
        """tdt_image_device_ptr: the address of the texels in device memory."""
        return int(lib().tdt_image_device_ptr(self.h) or 0)


class Program:
    """Uniform-by-name setters of program.rs:35-83 (the program object itself is the kernel)."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def set_i32(self, name, value):
        self.ctx.check(lib().tdt_set_i32(self.h, name.encode(), int(value)))

    def set_f32(self, name, value):
        self.ctx.check(lib().tdt_set_f32(self.h, name.encode(), float(value)))

    def set_vector3_f32(self, name, v):
        self.ctx.check(lib().tdt_set_vec3f(self.h, name.encode(), float(v[0]), float(v[1]), float(v[2])))

    def set_vector3_i32(self, name, v):
        self.ctx.check(lib().tdt_set_vec3i(self.h, name.encode(), int(v[0]), int(v[1]), int(v[2])))


class ComputeShader:
    """ComputeShader::new(program) / dispatch_compute(w, h, d) — compute_shader.rs:15-38."""

    def __init__(self, ctx, kind=PROGRAM_RAYTRACER):
        h = ctypes.c_void_p()
        ctx.check(lib().tdt_compute_create(ctx.h, kind, ctypes.byref(h)))
        self.ctx, self.h = ctx, h
        self.program = Program(ctx, h)
        gs = (ctypes.c_int * 3)()
        ctx.check(lib().tdt_compute_group_size(h, gs))
        self.group_size = list(gs)

    def dispatch_compute(self, width, height, depth):
        self.ctx.check(lib().tdt_dispatch_compute(self.h, width, height, depth))

    def pick(self, xy, sample=0, return_rays=False):
        """tdt_pick_pixels: what the primary ray of each pixel (x, y) — texture coordinates, row 0 at the bottom — and sample
        `sample` hits first, from this program's camera uniforms: numpy array of RAY_HIT_DTYPE (and the (n, 6) rays)."""
        p = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        out = np.zeros(p.shape[0], RAY_HIT_DTYPE)
        rays = np.zeros((p.shape[0], 6), np.float32) if return_rays else None
        self.ctx.check(lib().tdt_pick_pixels(self.h, p.ctypes.data, p.shape[0], int(sample),
                                             rays.ctypes.data if return_rays else None, out.ctypes.data))
        return (out, rays) if return_rays else out

    def dispatch_guide(self, texture, sample=0, all_materials=False):
        """tdt_dispatch_guide: texel (x, y) of `texture` (any Texture of the context, usually an unbound one) receives the surface
        key and depth of what the primary ray of pixel (x, y), sample `sample`, of this program's camera hits first — what pick
        returns for it, four words of it (Texture.read_guide).  Only Lambertian hits are keyed unless all_materials.  Asynchronous."""
        self.ctx.check(lib().tdt_dispatch_guide(self.h, texture.h, int(sample), GUIDE_ALL_MATERIALS if all_materials else 0))

    def dispatch_voxel_ids(self, texture, place=0, sample=0):
        """tdt_dispatch_voxel_ids: texel (x, y) of `texture` (any Texture of the context, usually an unbound one) receives the grid
        voxel a click on pixel (x, y) would act on — host.pick_grid_voxel of what pick returns for it: place=0 the voxel behind
        the face, place=1 the empty cell in front of it — as (state, Morton key, material, t) (Texture.read_voxel_ids).
        Asynchronous."""
        self.ctx.check(lib().tdt_dispatch_voxel_ids(self.h, texture.h, _place(place), int(sample)))

    def view(self):
        """tdt_compute_view: a VIEW snapshot of this program's current camera uniforms."""
        v = VIEW()
        self.ctx.check(lib().tdt_compute_view(self.h, ctypes.byref(v)))
        return v

    # --- extensions (no reference counterpart) ---
    def set_partition(self, rank, world):
        self.ctx.check(lib().tdt_set_partition(self.h, rank, world))

    def dispatch_accumulate(self, width, height, depth, spp_begin, spp_count, carry_ptr=None):
        self.ctx.check(lib().tdt_dispatch_accumulate(self.h, width, height, depth, spp_begin, spp_count,
                                                     ctypes.c_void_p(carry_ptr) if carry_ptr else None))

    def dispatch_accumulate_masked(self, width, height, depth, spp_begin, spp_count, carry_ptr, mask):
        """tdt_dispatch_accumulate_masked: dispatch_accumulate for the covered pixels whose texel of `mask` (a Texture of the bound
        image's size) has w >= 0; every other pixel keeps its texel and its carry.  A Texture.adapt state image is such a mask."""
        self.ctx.check(lib().tdt_dispatch_accumulate_masked(self.h, width, height, depth, spp_begin, spp_count,
                                                            ctypes.c_void_p(carry_ptr) if carry_ptr else None, mask.h))

    def dispatch_resolve(self, width, height, depth, total_spp):
        self.ctx.check(lib().tdt_dispatch_resolve(self.h, width, height, depth, total_spp))

    def covered_pixels(self, width, height, depth=1):
        return int(lib().tdt_covered_pixels(self.h, width, height, depth))

    def owned_tiles(self, width, height, depth=1):
        """(owned, tiles_per_row, total) 32x32 work-groups of a dispatch under the current partition."""
        tx, tot = ctypes.c_int(), ctypes.c_int()
        n = lib().tdt_owned_tiles(self.h, width, height, depth, ctypes.byref(tx), ctypes.byref(tot))
        return int(n), tx.value, tot.value

    def assemble_tiles(self, gathered_ptr, world, tiles_per_rank, dst_texture, width, height, depth=1):
        self.ctx.check(lib().tdt_assemble_tiles(self.h, ctypes.c_void_p(gathered_ptr), world, tiles_per_rank,
                                                dst_texture.h, width, height, depth))

    COUNT_FIELDS = ("pixels", "octree_hit_calls", "iterations", "node_loads", "lambertian", "metal", "dielectric",
                    "unknown_material")

    DEBUG_FIELDS = ("trav_slots", "trav_active", "level_slots", "level_active", "event_slots", "event_active",
                    "scatter_slots", "scatter_active", "memo_miss", "leaf_records")

    def debug_counters(self):
        c = (ctypes.c_uint64 * 32)()
        self.ctx.check(lib().tdt_debug_counters(self.ctx.h, c))
        d = dict(zip(self.DEBUG_FIELDS, [int(v) for v in c[8:18]]))
        d.update(first_start=int(c[18]), last_end=int(c[19]), sum_wave_cycles=int(c[20]), waves=int(c[21]), queue_empty=int(c[22]))
        d["region_cycles"] = dict(zip(("traverse", "gate", "hit_scatter", "end", "fetch", "primary", "newray"), [int(v) for v in c[24:31]]))
        return d

    def debug_wave_ends(self, n):
        c = (ctypes.c_uint64 * n)()
        self.ctx.check(lib().tdt_debug_wave_ends(self.ctx.h, c, n))
        return np.array(c, dtype=np.uint64)

    def debug_pixel_log(self, slots):
        """(slots, 8) uint32 per-pixel log of the last dispatch_counted; needs TDT_PIXEL_LOG in the environment."""
        log = np.zeros((slots, 8), np.uint32)
        self.ctx.check(lib().tdt_debug_pixel_log(self.ctx.h, log.ctypes.data, log.size))
        return log

    def dispatch_counted(self, width, height, depth=1):
        """Instrumented dispatch: event totals that define the algorithmic bytes."""
        c = (ctypes.c_uint64 * 8)()
        self.ctx.check(lib().tdt_dispatch_counted(self.h, width, height, depth, c))
        return dict(zip(self.COUNT_FIELDS, [int(v) for v in c]))

    def dispatch_counted_range(self, width, height, depth, spp_begin, spp_count, carry_ptr=None):
        """dispatch_accumulate, instrumented: the events of ONE launch of a progressive / two-phase frame."""
        c = (ctypes.c_uint64 * 8)()
        self.ctx.check(lib().tdt_dispatch_counted_range(self.h, width, height, depth, spp_begin, spp_count,
                                                        ctypes.c_void_p(carry_ptr) if carry_ptr else None, c))
        return dict(zip(self.COUNT_FIELDS, [int(v) for v in c]))


def trace_variants():
    """Every scene-specialised build of the trace kernel the library holds (tdt_debug_trace_variants): a list of
    (form, depth, resident, full, brick, unit) tuples in Context.last_variant's field order.  Needs no device."""
    n = ctypes.c_int(0)
    rc = lib().tdt_debug_trace_variants(None, 0, ctypes.byref(n))
    if rc != 0:
        raise TdtError(rc, "tdt_debug_trace_variants")
    rows = (ctypes.c_int * (6 * n.value))()
    rc = lib().tdt_debug_trace_variants(rows, n.value, ctypes.byref(n))
    if rc != 0:
        raise TdtError(rc, "tdt_debug_trace_variants")
    return [tuple(int(x) for x in rows[6 * i:6 * i + 6]) for i in range(n.value)]


def octree_build_cells(ctx, voxels_xyzm, depth):
    """SURVEY §8f-1 on the GPU (tdt_octree_build_cells): (n, 4) int32 voxels {x, y, z, material + 1} in grid coordinates ->
    (cells VertexBufferObject, number of cells)."""
    v = np.ascontiguousarray(voxels_xyzm, np.int32).reshape(-1, 4)
    h, n = ctypes.c_void_p(), ctypes.c_uint32(0)
    ctx.check(lib().tdt_octree_build_cells(ctx.h, v.ctypes.data if v.size else None, v.shape[0], depth, ctypes.byref(h), ctypes.byref(n)))
    return VertexBufferObject._adopt(ctx, h, int(n.value) * 64), int(n.value)


def octree_build_from_points(ctx, voxels_xyzk, min_point, palette_keys, palette_rgb, z_up=True, max_iter=256):
    """tdt_scene_from_ply on the GPU (tdt_octree_build_from_points): PlyFileContent{voxels, albedos, min_point}
    (ply_point_loader.rs:84-93) -> ({slot: VertexBufferObject} for slots 0,1,2,3,4,6,7 — not bound —, max_depth, cell_count)."""
    v = np.ascontiguousarray(voxels_xyzk, np.int32).reshape(-1, 4)
    keys = np.ascontiguousarray(palette_keys, np.uint32)
    rgb = np.ascontiguousarray(palette_rgb, np.uint8).reshape(-1, 3)
    mp = (ctypes.c_int32 * 3)(*[int(x) for x in min_point])
    out = (ctypes.c_void_p * 8)()
    depth, cc = ctypes.c_int32(0), ctypes.c_int32(0)
    ctx.check(lib().tdt_octree_build_from_points(ctx.h, v.ctypes.data, v.shape[0], mp, keys.ctypes.data, rgb.ctypes.data, keys.size,
                                                 1 if z_up else 0, max_iter, out, ctypes.byref(depth), ctypes.byref(cc)))
    vbos = {}
    for slot in (0, 1, 2, 3, 4, 6, 7):
        vbos[slot] = VertexBufferObject._adopt(ctx, ctypes.c_void_p(out[slot]), 0)
    return vbos, int(depth.value), int(cc.value)


def initial_uniforms(camera, program):
    """camera.rs:241-253: sends all eight camera uniforms."""
    program.set_i32("camera.image_width", camera.image_width)
    program.set_i32("camera.image_height", camera.image_height)
    program.set_vector3_f32("camera.horizontal", camera.horizontal)
    program.set_vector3_f32("camera.vertical", camera.vertical)
    program.set_vector3_f32("camera.lower_left_corner", camera.lower_left_corner)
    program.set_vector3_f32("camera.origin", camera.origin)
    program.set_i32("camera.samples_per_pixel", camera.samples_per_pixel)
    program.set_i32("camera.max_bounce", camera.max_bounce)


def update_vbo(ctx, delta_vbo, delta, length, update_compute):
    """Octree::update_vbo (octree.rs:170-183): BufferSubData of `length` floats, then the oddly shaped
    dispatch — (0, n, 0) unless n / 1024 is integral, n = (length as f32 * 0.2) as i32."""
    d = np.ascontiguousarray(delta, np.float32)[:length]
    delta_vbo.sub_data(0, d)
    x_schedule = np.float32(length) * np.float32(0.2)
    dispatch_count = int(x_schedule)
    q = x_schedule / np.float32(32.0 * 32.0)
    if q - np.trunc(q) != 0:
        update_compute.dispatch_compute(0, dispatch_count, 0)
    else:
        update_compute.dispatch_compute(dispatch_count, 1, 1)


def upload_scene(ctx, scene):
    """What main.rs:343-450 and Octree::init_global_buffers (octree.rs:44-100) do: one buffer per
    payload, bound to its shader-storage slot.  Returns the buffers (keep them alive)."""
    vbos = {}
    for slot in (0, 1, 2, 3, 4, 6, 7):
        vbos[slot] = VertexBufferObject(ctx, scene.blobs[slot])
        ctx.bind_buffer_base(SHADER_STORAGE_BUFFER, slot, vbos[slot])
    return vbos


# Renderer.render_temporal's sample indices stay below this.  primary_ray hashes fract(K * (x + (float)sample)) with K = 0.02062:
# up to 2^20 the float spacing of that product (2^-9) is far below K, so consecutive samples still get different jitter; near
# 2^24 they would coincide, and k * spp as a C int would overflow later still.
TEMPORAL_SAMPLE_PERIOD = 1 << 20
# The sigma of Texture.denoise_variance that DESIGN.md's quality table recommends: renderer.variance = VARIANCE_SIGMA.
VARIANCE_SIGMA = 4.0


class Renderer:
    """Convenience wrapper used by tests, smoke() and bench.py: a context with one scene, one
    camera and one image, i.e. the state main.rs has built when it reaches its render loop."""

    def __init__(self, scene, camera, device=0, stream=None, rank=0, world=1, image_ptr=None, tile_buffer_tiles=None, devices=None):
        self.ctx = Context(device, stream, devices=devices)
        self.shader = ComputeShader(self.ctx)
        self.vbos = upload_scene(self.ctx, scene)
        self.camera = camera
        initial_uniforms(camera, self.shader.program)
        if devices is None:
            self.shader.set_partition(rank, world)
        if tile_buffer_tiles is not None:      # this rank's tile buffer [k][32][32] RGBA
            w, rows = 32, 32 * tile_buffer_tiles
        else:
            w, rows = camera.image_width, camera.image_height
        if image_ptr is not None:
            self.texture = Texture.wrap_device(self.ctx, image_ptr, w, rows)
        else:
            self.texture = Texture.new_2d(self.ctx, w, rows)
        self.guide = None                      # render(denoise=N) creates it on first use
        self.temporal = None                   # render_temporal's state, created on first use
        self.low = None                        # render_upsampled's low-resolution (sums, guide) textures, created on first use
        self.adaptive = None                   # render_adaptive's two state textures and its carry, created on first use
        self.ids = None                        # render_overlay's and select_rect's voxel-id texture, created on first use
        self.adaptive_floor = 0.05            # render_adaptive: the brightness below which the error is measured against this value
        # sigma of the variance-guided filter that render(denoise=N) and render_temporal(denoise=N) run instead of the key-only one;
        # None: the key-only filter, exactly the calls made before the variance unit existed.  VARIANCE_SIGMA is the measured default.
        self.variance = None
        self.variance_min_frames = 4.0         # render_temporal: frames behind a pixel from which its temporal variance is trusted

    def dispatch(self, width=None, height=None):
        """main.rs:579: dispatch_compute(texture.width() + 1, texture.height() + 1, 1)."""
        w = self.camera.image_width + 1 if width is None else width
        h = self.camera.image_height + 1 if height is None else height
        self.shader.dispatch_compute(w, h, 1)

    def render(self, width=None, height=None, denoise=0):
        """The frame.  denoise = N > 0: the same samples as running sums (dispatch_accumulate), the first-hit guide of sample 0,
        N filter passes over the sums, then the resolve — the square root is taken of the filtered sums.  With self.variance =
        SIGMA the passes are the variance-guided ones (Texture.variance's spatial estimate, then Texture.denoise_variance with that
        sigma); None, the default: the key-only filter."""
        if denoise > 0:
            w = self.camera.image_width + 1 if width is None else width
            h = self.camera.image_height + 1 if height is None else height
            spp = self.camera.samples_per_pixel
            if self.guide is None:
                self.guide = Texture.new_2d(self.ctx, self.texture.width(), self.texture.height(), bind=False)
            self.shader.dispatch_accumulate(w, h, 1, 0, spp)
            self.shader.dispatch_guide(self.guide)
            if self.variance is None:
                self.texture.denoise(self.guide, denoise)
            else:
                self.texture.variance(self.guide)
                self.texture.denoise_variance(self.guide, denoise, self.variance)
            self.shader.dispatch_resolve(w, h, 1, spp)
            return self.texture.read()
        self.dispatch(width, height)
        return self.texture.read()

    def render_temporal(self, width=None, height=None, cam=None, denoise=0, max_samples=64.0, reset=False):
        """One frame of an interactive sequence, with the samples of earlier frames reprojected into it (Texture.reproject).  Frame k
        traces samples [k spp, (k+1) spp) of the camera's samples_per_pixel, takes the guide of sample k spp, adds the history of the
        frame before wherever that frame saw the same surface point (at most max_samples of it), filters the means with `denoise`
        passes and resolves them.  cam, when given, becomes the renderer's camera (the camera moved); reset drops the history and
        starts again at frame 0 — after a scene edit, whose lighting change nothing here detects.  The renderer owns the frame
        counter, the two history and the two guide textures and the previous view.  The sample index wraps to 0 every
        TEMPORAL_SAMPLE_PERIOD // spp frames (the history is kept): a session of any length stays inside the range in which the
        sampler tells samples apart.  With self.variance = SIGMA and denoise > 0 the frames also carry luminance moments
        (Texture.reproject_moments; two more textures, created when first asked for), Texture.variance takes the temporal estimate
        where a pixel has enough frames and the spatial one elsewhere, and the passes are Texture.denoise_variance's; asked for in
        the middle of a sequence, the moments start at that frame.  Returns the resolved frame.  A single-device
        renderer whose image is the whole frame only: on several devices the running sums live in per-device tile buffers."""
        if self.ctx.device_count() != 1 or self.texture.width() != self.camera.image_width or self.texture.height() != self.camera.image_height:
            raise ValueError("render_temporal needs a single-device renderer that owns the whole image")
        if cam is not None:
            if (cam.image_width, cam.image_height) != (self.camera.image_width, self.camera.image_height):
                raise ValueError("render_temporal keeps one image size: the new camera's differs")
            self.camera = cam
            initial_uniforms(cam, self.shader.program)
        w = self.camera.image_width + 1 if width is None else width
        h = self.camera.image_height + 1 if height is None else height
        spp = self.camera.samples_per_pixel
        t = self.temporal
        if t is None:
            new = lambda: Texture.new_2d(self.ctx, self.texture.width(), self.texture.height(), bind=False)  # noqa: E731
            t = self.temporal = {"frame": 0, "view": None, "hist": (new(), new()), "guide": (new(), new())}
        if reset:
            t["frame"], t["view"] = 0, None
        k = t["frame"]
        cur, old = k & 1, (k & 1) ^ 1
        sample = (k % max(1, TEMPORAL_SAMPLE_PERIOD // spp)) * spp
        if sample:
            self.texture.clear()               # (a range that starts past sample 0 is added to what the image holds)
        self.shader.dispatch_accumulate(w, h, 1, sample, spp)
        self.shader.dispatch_guide(t["guide"][cur], sample=sample)
        prev = (t["view"], t["guide"][old], t["hist"][old]) if t["view"] is not None else None
        if self.variance is not None and denoise > 0:
            if "moments" not in t:
                t["moments"] = (Texture.new_2d(self.ctx, self.texture.width(), self.texture.height(), bind=False),
                                Texture.new_2d(self.ctx, self.texture.width(), self.texture.height(), bind=False))
                t["moments_live"] = False
            if not t["moments_live"]:
                t["moments"][old].clear()              # (the frame before wrote none: frame count 0, nothing behind this one)
            self.texture.reproject_moments(self.shader, sample, t["guide"][cur], spp, prev + (t["moments"][old],) if prev is not None else None,
                                           max_samples, hist_out=t["hist"][cur], moments_out=t["moments"][cur], mean_out=self.texture)
            self.texture.variance(t["guide"][cur], t["moments"][cur], self.variance_min_frames)
            self.texture.denoise_variance(t["guide"][cur], denoise, self.variance)
            t["moments_live"] = True
        else:
            t["moments_live"] = False                  # (a frame without moments breaks their sequence)
            self.texture.reproject(self.shader, sample, t["guide"][cur], spp, prev, max_samples, hist_out=t["hist"][cur], mean_out=self.texture)
            if denoise > 0:
                self.texture.denoise(t["guide"][cur], denoise)
        self.shader.dispatch_resolve(w, h, 1, 1)
        t["view"], t["frame"] = self.shader.view(), k + 1
        return self.texture.read()

    def render_upsampled(self, scale=2, denoise=0, width=None, height=None):
        """The frame with its radiance traced at 1 / scale of the resolution (Texture.upsample).  The low camera is the renderer's
        with only image_width = ceil(W / scale) and image_height = ceil(H / scale) changed — the same frustum.  The frame: under
        the low uniforms, with a low texture bound, accumulate [0, spp) over the whole low image and take the low guide of sample 0;
        under the full uniforms the full guide of sample 0; upsample into the renderer's texture; `denoise` > 0: the filter calls
        render(denoise=N) makes (self.variance decides which); bind the renderer's texture and resolve with spp.  width / height are
        the resolve's dispatch, as render's.  scale=1 goes through the same calls.  The low texture and the two guides are created
        on first use.  A single-device renderer whose image is the whole frame only; whether it returns or raises, the uniforms and
        the binding are the full-resolution ones afterwards.  Returns the resolved frame."""
        if isinstance(scale, bool) or not isinstance(scale, int) or scale < 1:
            raise ValueError("render_upsampled: scale must be an int >= 1")
        W, H = self.camera.image_width, self.camera.image_height
        if self.ctx.device_count() != 1 or self.texture.width() != W or self.texture.height() != H:
            raise ValueError("render_upsampled needs a single-device renderer that owns the whole image")
        w = W + 1 if width is None else width
        h = H + 1 if height is None else height
        spp = self.camera.samples_per_pixel
        lw, lh = -(-W // scale), -(-H // scale)
        if self.guide is None:
            self.guide = Texture.new_2d(self.ctx, W, H, bind=False)
        if self.low is None or (self.low[0].width(), self.low[0].height()) != (lw, lh):
            self.low = (Texture.new_2d(self.ctx, lw, lh, bind=False), Texture.new_2d(self.ctx, lw, lh, bind=False))
        low, low_guide = self.low
        program = self.shader.program
        try:
            program.set_i32("camera.image_width", lw)
            program.set_i32("camera.image_height", lh)
            low.bind()
            self.shader.dispatch_accumulate(-(-lw // 32) * 32, -(-lh // 32) * 32, 1, 0, spp)    # (work-groups over all of the low image)
            self.shader.dispatch_guide(low_guide)
        finally:
            program.set_i32("camera.image_width", W)
            program.set_i32("camera.image_height", H)
            self.texture.bind()
        self.shader.dispatch_guide(self.guide)
        self.texture.upsample(self.guide, low, low_guide)
        if denoise > 0:
            if self.variance is None:
                self.texture.denoise(self.guide, denoise)
            else:
                self.texture.variance(self.guide)
                self.texture.denoise_variance(self.guide, denoise, self.variance)
        self.shader.dispatch_resolve(w, h, 1, spp)
        return self.texture.read()

    def render_adaptive(self, tolerance, batch=2, min_samples=4, max_samples=None, denoise=0):
        """The frame with its samples spent where the image is still noisy (ComputeShader.dispatch_accumulate_masked, Texture.adapt).
        Clear the texture, one state texture and the carry; then rounds of `batch` samples for the pixels still live, each followed
        by Texture.adapt (with the guide of sample 0, taken once) and a read of its counts, until nothing is live — at the latest
        when every live pixel has max_samples (None: the camera's samples_per_pixel).  Then Texture.adapt_mean, `denoise` > 0: the
        filter calls render(denoise=N) makes (self.variance decides which; the variance-guided filter reads the batch-mean variance
        adapt_mean left in alpha), and the resolve with total_spp = 1.  Every pixel ends with a prefix [0, n) of the sample
        sequence, n a multiple of batch; self.adaptive["samples"]() reads the last call's per-pixel sample counts, ["rounds"] its rounds.  A
        single-device renderer whose image is the whole frame only.  Returns the resolved frame."""
        W, H = self.camera.image_width, self.camera.image_height
        if self.ctx.device_count() != 1 or self.texture.width() != W or self.texture.height() != H:
            raise ValueError("render_adaptive needs a single-device renderer that owns the whole image")
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError("render_adaptive: batch must be an int >= 1")
        cap = self.camera.samples_per_pixel if max_samples is None else max_samples
        if isinstance(cap, bool) or not isinstance(cap, int) or cap < 1:
            raise ValueError("render_adaptive: max_samples must be an int >= 1")
        w, h = W + 1, H + 1
        if self.guide is None:
            self.guide = Texture.new_2d(self.ctx, W, H, bind=False)
        if self.adaptive is None:
            new = lambda cols: Texture.new_2d(self.ctx, cols, H, bind=False)  # noqa: E731
            self.adaptive = {"state": (new(W), new(W)), "carry": new(4 * W)}      # (the carry: 16 floats per pixel = four texels)
        t = self.adaptive
        cur, other = t["state"]
        self.texture.clear()
        cur.clear()
        t["carry"].clear()
        carry = t["carry"].device_ptr()
        begin, rounds = 0, 0
        while True:
            self.shader.dispatch_accumulate_masked(w, h, 1, begin, batch, carry, cur)
            if rounds == 0:
                self.shader.dispatch_guide(self.guide)
            self.texture.adapt(self.guide, cur, other, batch, tolerance, self.adaptive_floor, min_samples, cap)
            cur, other = other, cur
            begin += batch
            rounds += 1
            if self.ctx.adapt_counts()[3] == 0:
                break
        t["state"] = (cur, other)
        t["rounds"] = rounds
        t["samples"] = lambda: np.abs(cur.read()[..., 3]).astype(np.int64)
        self.texture.adapt_mean(cur)
        if denoise > 0:
            if self.variance is None:
                self.texture.denoise(self.guide, denoise)
            else:
                self.texture.denoise_variance(self.guide, denoise, self.variance)
        self.shader.dispatch_resolve(w, h, 1, 1)
        return self.texture.read()

    def _ids_texture(self):
        """The voxel-id texture of render_overlay and select_rect, of the renderer's texture's size, created on first use."""
        if self.ids is None:
            self.ids = Texture.new_2d(self.ctx, self.texture.width(), self.texture.height(), bind=False)
        return self.ids

    def render_overlay(self, voxels, place=0, fill=(1, .6, 0, .35), edge=(1, .6, 0, 1), edge_width=1, voxel_edges=False, width=None,
                       height=None, denoise=0):
        """The frame with a voxel list drawn over it — the preview of an edit that has not been applied: render(width, height,
        denoise), the voxel ids of sample 0 (ComputeShader.dispatch_voxel_ids with `place`), Texture.overlay of `voxels` over the
        resolved frame.  First hit only: voxels of the list that something hides are not shown.  Returns (frame, ids), ids being
        Texture.read_voxel_ids() of the frame's id image; while camera and tree stay as they are, another list needs only
        render + self.texture.overlay(self.ids, ..).  A renderer whose image is the whole frame only."""
        style = _overlay(fill, edge, edge_width, voxel_edges)
        place = _place(place)
        v = np.ascontiguousarray(np.asarray(voxels, np.int32).reshape(-1, 4))
        if self.texture.width() != self.camera.image_width or self.texture.height() != self.camera.image_height:
            raise ValueError("render_overlay needs a renderer that owns the whole image")
        self.render(width, height, denoise)
        ids = self._ids_texture()
        self.shader.dispatch_voxel_ids(ids, place, 0)
        self.texture.overlay(ids, v, style.fill[:], style.edge[:], style.edge_width, voxel_edges)
        return self.texture.read(), ids.read_voxel_ids()

    def select_rect(self, rect, place=0, sample=0):
        """Marquee selection: the distinct voxels visible inside rect = (x0, y0, x1, y1) (inclusive pixel coordinates, row 0 at
        the bottom, clipped to the image) — for every pixel the voxel a click there would act on (`place`, `sample` as
        ComputeShader.dispatch_voxel_ids takes them) — as an (n, 4) int32 list {x, y, z, material + 1}, Morton-sorted: what
        Context.octree_edit_voxels takes.  A renderer whose image is the whole frame only."""
        if rect is None or len(rect) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in rect):
            raise ValueError("select_rect: rect is four ints (x0, y0, x1, y1)")
        place = _place(place)
        if isinstance(sample, bool) or not isinstance(sample, (int, np.integer)) or sample < 0:
            raise ValueError("select_rect: sample must be an int >= 0")
        if self.texture.width() != self.camera.image_width or self.texture.height() != self.camera.image_height:
            raise ValueError("select_rect needs a renderer that owns the whole image")
        ids = self._ids_texture()
        self.shader.dispatch_voxel_ids(ids, place, int(sample))
        return ids.extract_voxels(rect)

    def select_through(self, rect=None, polygon=None, mask=None, **filters):
        """The marquee that selects through the model: every voxel of the scene that projects, under the renderer's current
        camera (ComputeShader.view), into rect = (x0, y0, x1, y1), the lasso `polygon` or the Texture `mask` — hidden or not, unlike
        select_rect — with Context.octree_extract_screen's filters (window, material, min_distance, max_distance), as an (n, 4)
        int32 list {x, y, z, material + 1}, Morton-sorted: what Context.octree_edit_voxels and render_overlay take."""
        unknown = set(filters) - {"window", "material", "min_distance", "max_distance"}
        if unknown:
            raise ValueError("select_through: unknown filter " + ", ".join(sorted(unknown)))
        _screen_select(rect, polygon, mask, filters.get("window", False), filters.get("material"), filters.get("min_distance", 0.0),
                       filters.get("max_distance", float("inf")))
        return self.ctx.octree_extract_screen(self.shader.view(), rect=rect, polygon=polygon, mask=mask, **filters)

    def pick(self, xy, sample=0, return_rays=False):
        """ComputeShader.pick with this renderer's camera: what is under each pixel."""
        return self.shader.pick(xy, sample, return_rays)

    def stroke(self, pixels, radius, op, material=0, shape=SHAPE_SPHERE, sample=0):
        """A brush dragged over the pixels (n, 2) of this renderer's camera: one batched pick of all of them, each hit turned into
        the grid voxel in front of the face (REGION_SET / REGION_FILL) or behind it (REGION_PAINT / REGION_CLEAR)
        (host.pick_grid_voxel), consecutive hits joined by segments, a miss breaking the stroke and a hit between two misses
        left as a dab; then Context.octree_edit_stroke of those points and segments.  Returns (points, cells): the (k, 3) int32
        points used and the canonical tree's cell count.  No hit at all: the empty stroke, which installs the compacted tree."""
        from . import host
        hits = self.pick(pixels, sample)
        place = 1 if op in (REGION_SET, REGION_FILL) else 0
        uniforms = (self.vbos[6].read(np.float32), self.vbos[7].read(np.int32))   # slots 6 / 7 as the device holds them
        points, segments, prev = [], [], None
        for h in hits:
            try:
                v = host.pick_grid_voxel(h, uniforms, place)
            except ValueError:                             # a miss, a stale record or a point outside the octree
                prev = None
                continue
            points.append(v)
            if prev is not None:
                segments.append((prev, len(points) - 1))
            prev = len(points) - 1
        joined = {i for g in segments for i in g}
        segments += [(i, i) for i in range(len(points)) if i not in joined]
        pts = np.asarray(points, np.int32).reshape(-1, 3)
        seg = np.asarray(segments, np.uint32).reshape(-1, 2)
        return pts, self.ctx.octree_edit_stroke(op, pts, radius, segments=seg, material=material, shape=shape)

    def extrude(self, pixel, distance, op, material=-1, connectivity=4, match=MATCH_MATERIAL, block=False, sample=0):
        """The face under `pixel` = (x, y) of this renderer's camera pulled out, pushed in or painted: one pick, the hit turned
        into the seed {x, y, z, f} (host.pick_face), then Context.octree_edit_faces of the face region that holds it swept by the
        signed `distance` — REGION_FILL / REGION_SET with distance > 0 pulls, REGION_CLEAR with distance < 0 pushes,
        REGION_PAINT with distance -1 paints.  Returns (seed, cells): the (4,) int32 seed and the canonical tree's cell count.  A
        pixel that hits nothing raises ValueError."""
        from . import host
        _faces(np.zeros((0, 4), np.int32), distance, connectivity, match, block, material, op=op)
        hit = self.pick([pixel], sample)[0]
        uniforms = (self.vbos[6].read(np.float32), self.vbos[7].read(np.int32))   # slots 6 / 7 as the device holds them
        seed = host.pick_face(hit, uniforms)                                      # a miss, a stale record: ValueError
        return seed, self.ctx.octree_edit_faces(op, seed.reshape(1, 4), distance, connectivity, match, block, material)

    def compact(self):
        """Context.octree_compact on this renderer's scene: the number of cells the canonical tree takes."""
        return self.ctx.octree_compact()

    def close(self):
        self.ctx.close()
