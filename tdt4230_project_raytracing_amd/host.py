"""ctypes binding of libtdthost.so (include/tdt_host.h): camera uniforms and scene payloads.

Host-side restatement of the reference's Rust host code — CameraBuilder::build
(src/renderer/camera.rs:135-196), Octree::init_global_buffers (src/renderer/octree.rs:40-100),
the demo scene literal (src/main.rs:235-463) — plus the synthetic-scene generators.  Pure
host code; no HIP, no oracle.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libtdthost.so")

SLOTS = (0, 1, 2, 3, 4, 6, 7)
SLOT_DTYPES = {0: np.uint32, 1: np.uint32, 2: np.float32, 3: np.float32, 4: np.float32, 6: np.float32, 7: np.int32}
SLOT_NAMES = {0: "cells", 1: "materials", 2: "albedos", 3: "metal", 4: "dielectric", 6: "octree_floats", 7: "octree_ints"}


class CameraBuilderC(ctypes.Structure):
    _fields_ = [
        ("vertical_fov", ctypes.c_float), ("image_width", ctypes.c_int32),
        ("has_aspect_ratio", ctypes.c_int32), ("aspect_ratio", ctypes.c_float),
        ("has_viewport_height", ctypes.c_int32), ("viewport_height", ctypes.c_float),
        ("has_origin", ctypes.c_int32), ("origin", ctypes.c_float * 3),
        ("has_samples_per_pixel", ctypes.c_int32), ("samples_per_pixel", ctypes.c_int32),
        ("has_max_bounce", ctypes.c_int32), ("max_bounce", ctypes.c_int32),
        ("has_turn_rate", ctypes.c_int32), ("turn_rate", ctypes.c_float),
        ("has_normal_speed", ctypes.c_int32), ("normal_speed", ctypes.c_float),
        ("has_sprint_speed", ctypes.c_int32), ("sprint_speed", ctypes.c_float),
    ]


class CameraUniforms(ctypes.Structure):
    """`uniform Camera camera` (raytracer.comp:133-146) as initial_uniforms sends it (camera.rs:241-253)."""
    _fields_ = [
        ("image_width", ctypes.c_int32), ("image_height", ctypes.c_int32),
        ("horizontal", ctypes.c_float * 3), ("vertical", ctypes.c_float * 3),
        ("lower_left_corner", ctypes.c_float * 3), ("origin", ctypes.c_float * 3),
        ("samples_per_pixel", ctypes.c_int32), ("max_bounce", ctypes.c_int32),
    ]

    def copy(self):
        c = CameraUniforms()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(self), ctypes.sizeof(self))
        return c


class CameraSettings(ctypes.Structure):
    """CameraSettings (camera.rs:9-16) = assets/settings/camera.ron."""
    _fields_ = [("samples_per_pixel", ctypes.c_int32), ("max_bounce", ctypes.c_int32), ("turn_rate", ctypes.c_float),
                ("normal_speed", ctypes.c_float), ("sprint_speed", ctypes.c_float)]

    @classmethod
    def from_ron(cls, text):
        """ron::de::from_bytes::<CameraSettings> (main.rs:171, 493)."""
        data = text.encode() if isinstance(text, str) else bytes(text)
        out = cls()
        _check(lib().tdt_camera_settings_from_ron(data, len(data), ctypes.byref(out)))
        return out


class CameraC(ctypes.Structure):
    _fields_ = [("horizontal", ctypes.c_float * 3), ("vertical", ctypes.c_float * 3),
                ("viewport_width", ctypes.c_float), ("viewport_height", ctypes.c_float),
                ("lower_left_corner", ctypes.c_float * 3), ("origin", ctypes.c_float * 3),
                ("pitch", ctypes.c_float * 4), ("yaw", ctypes.c_float * 4),
                ("image_width", ctypes.c_int32), ("image_height", ctypes.c_int32),
                ("settings", CameraSettings), ("movement_speed", ctypes.c_float)]


# Direction::into_vector3 (utility/mod.rs:15-26)
DIRECTION = {"Front": (0.0, 0.0, -1.0), "Back": (0.0, 0.0, 1.0), "Rigth": (1.0, 0.0, 0.0), "Left": (-1.0, 0.0, 0.0),
             "Up": (0.0, 1.0, 0.0), "Down": (0.0, -1.0, 0.0)}


class Camera:
    """The reference's Camera (camera.rs:20-102) without the GL objects: the controller state and the uniforms it sends
    (cgmath restated, parity unpinned — see include/tdt_host.h)."""

    def __init__(self, vertical_fov, image_width, aspect_ratio=None, viewport_height=None, origin=None, samples_per_pixel=None,
                 max_bounce=None, turn_rate=None, normal_speed=None, sprint_speed=None):
        b = _builder(vertical_fov, image_width, aspect_ratio, viewport_height, origin, samples_per_pixel, max_bounce)
        for name, v in (("turn_rate", turn_rate), ("normal_speed", normal_speed), ("sprint_speed", sprint_speed)):
            if v is not None:
                setattr(b, "has_" + name, 1)
                setattr(b, name, v)
        self.c = CameraC()
        _check(lib().tdt_camera_init(ctypes.byref(b), ctypes.byref(self.c)))

    def translate(self, by, deltatime):
        v = (ctypes.c_float * 3)(*(DIRECTION[by] if isinstance(by, str) else by))
        _check(lib().tdt_camera_translate(ctypes.byref(self.c), v, ctypes.c_double(deltatime)))

    def turn_pitch(self, angle):
        _check(lib().tdt_camera_turn_pitch(ctypes.byref(self.c), ctypes.c_float(angle)))

    def turn_yaw(self, angle):
        _check(lib().tdt_camera_turn_yaw(ctypes.byref(self.c), ctypes.c_float(angle)))

    def set_speed_to_normal(self):
        lib().tdt_camera_set_speed_to_normal(ctypes.byref(self.c))

    def set_speed_to_sprint(self):
        lib().tdt_camera_set_speed_to_sprint(ctypes.byref(self.c))

    def look_at_world_point(self, distance):
        out = (ctypes.c_float * 3)()
        _check(lib().tdt_camera_look_at_world_point(ctypes.byref(self.c), ctypes.c_float(distance), out))
        return list(out)

    def apply_settings(self, settings):
        _check(lib().tdt_camera_apply_settings(ctypes.byref(self.c), ctypes.byref(settings)))

    def uniforms(self):
        u = CameraUniforms()
        _check(lib().tdt_camera_get_uniforms(ctypes.byref(self.c), ctypes.byref(u)))
        return u


# ---------------------------------------------------------------- presentation ---
def present_rgba8(image, top_down=True):
    """What the reference's quad pass leaves in an RGBA8 back buffer (quad.frag:10, main.rs:582-600) for an (H, W, 4) float32
    render texture with row 0 at the bottom; host-side counterpart of rt.Texture.read_rgba8."""
    image = np.ascontiguousarray(image, np.float32)
    h, w = image.shape[:2]
    out = np.empty((h, w, 4), np.uint8)
    _check(lib().tdt_present_rgba8(image.ctypes.data, w, h, 1 if top_down else 0, out.ctypes.data))
    return out


def png_encode(rgba8, with_alpha=False):
    """8-bit PNG bytes of a top-down (H, W, 4) uint8 frame."""
    rgba8 = np.ascontiguousarray(rgba8, np.uint8)
    h, w = rgba8.shape[:2]
    buf, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    _check(lib().tdt_png_encode(rgba8.ctypes.data, w, h, 1 if with_alpha else 0, ctypes.byref(buf), ctypes.byref(n)))
    try:
        return ctypes.string_at(buf, n.value)
    finally:
        lib().tdt_host_free(buf)


def png_write(path, rgba8, with_alpha=False):
    rgba8 = np.ascontiguousarray(rgba8, np.uint8)
    h, w = rgba8.shape[:2]
    _check(lib().tdt_png_write(os.fsencode(path), rgba8.ctypes.data, w, h, 1 if with_alpha else 0))


class SceneParams(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("max_depth", ctypes.c_int32), ("cell_count", ctypes.c_int32),
                ("max_iter", ctypes.c_int32), ("seed", ctypes.c_uint64)]


SCENE_HASH_GRID, SCENE_TERRAIN, SCENE_SHELLS = 0, 1, 2

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(_LIB_PATH)
        L.tdt_host_last_error.restype = ctypes.c_char_p
        L.tdt_camera_build.argtypes = [ctypes.POINTER(CameraBuilderC), ctypes.POINTER(CameraUniforms)]
        L.tdt_camera_reference_pose.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(CameraUniforms)]
        L.tdt_scene_demo.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        L.tdt_scene_generate.argtypes = [ctypes.POINTER(SceneParams), ctypes.POINTER(ctypes.c_void_p)]
        L.tdt_scene_config.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.tdt_scene_from_blobs.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                           ctypes.POINTER(ctypes.c_void_p)]
        L.tdt_scene_destroy.argtypes = [ctypes.c_void_p]
        L.tdt_scene_destroy.restype = None
        L.tdt_scene_blob.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
        L.tdt_scene_blob.restype = ctypes.c_void_p
        L.tdt_scene_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
        L.tdt_camera_init.argtypes = [ctypes.POINTER(CameraBuilderC), ctypes.POINTER(CameraC)]
        L.tdt_camera_translate.argtypes = [ctypes.POINTER(CameraC), ctypes.POINTER(ctypes.c_float), ctypes.c_double]
        L.tdt_camera_turn_pitch.argtypes = [ctypes.POINTER(CameraC), ctypes.c_float]
        L.tdt_camera_turn_yaw.argtypes = [ctypes.POINTER(CameraC), ctypes.c_float]
        L.tdt_camera_set_speed_to_normal.argtypes = [ctypes.POINTER(CameraC)]
        L.tdt_camera_set_speed_to_normal.restype = None
        L.tdt_camera_set_speed_to_sprint.argtypes = [ctypes.POINTER(CameraC)]
        L.tdt_camera_set_speed_to_sprint.restype = None
        L.tdt_camera_look_at_world_point.argtypes = [ctypes.POINTER(CameraC), ctypes.c_float, ctypes.POINTER(ctypes.c_float)]
        L.tdt_camera_apply_settings.argtypes = [ctypes.POINTER(CameraC), ctypes.POINTER(CameraSettings)]
        L.tdt_camera_get_uniforms.argtypes = [ctypes.POINTER(CameraC), ctypes.POINTER(CameraUniforms)]
        L.tdt_camera_settings_from_ron.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(CameraSettings)]
        L.tdt_present_rgba8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.tdt_png_encode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                     ctypes.POINTER(ctypes.c_size_t)]
        L.tdt_png_write.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.tdt_host_free.argtypes = [ctypes.c_void_p]
        L.tdt_host_free.restype = None
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError("libtdthost: " + lib().tdt_host_last_error().decode())


class Scene:
    """The seven SSBO payloads of one scene, as numpy arrays (copies) keyed by binding slot."""

    def __init__(self, blobs, counts=None, name=""):
        self.blobs = {int(k): np.ascontiguousarray(v) for k, v in blobs.items()}
        self.counts = counts
        self.name = name

    @classmethod
    def _from_handle(cls, h, name):
        L = lib()
        blobs = {}
        for slot in SLOTS:
            n = ctypes.c_size_t(0)
            p = L.tdt_scene_blob(h, slot, ctypes.byref(n))
            dt = np.dtype(SLOT_DTYPES[slot])
            if n.value:
                buf = (ctypes.c_char * n.value).from_address(p)
                blobs[slot] = np.frombuffer(buf, dtype=dt).copy()
            else:
                blobs[slot] = np.zeros(0, dt)
        cnt = (ctypes.c_int64 * 6)()
        _check(L.tdt_scene_counts(h, cnt))
        L.tdt_scene_destroy(h)
        keys = ("cells", "parents", "leaves", "empties", "materials", "voxels")
        return cls(blobs, dict(zip(keys, list(cnt))), name)

    @classmethod
    def demo(cls):
        h = ctypes.c_void_p()
        _check(lib().tdt_scene_demo(ctypes.byref(h)))
        return cls._from_handle(h, "demo")

    @classmethod
    def config(cls, n):
        h = ctypes.c_void_p()
        _check(lib().tdt_scene_config(int(n), ctypes.byref(h)))
        return cls._from_handle(h, f"config{n}")

    @classmethod
    def generate(cls, kind, max_depth, cell_count, max_iter, seed):
        p = SceneParams(kind, max_depth, cell_count, max_iter, seed)
        h = ctypes.c_void_p()
        _check(lib().tdt_scene_generate(ctypes.byref(p), ctypes.byref(h)))
        return cls._from_handle(h, f"gen{kind}_d{max_depth}_s{seed:x}")

    @property
    def max_depth(self):
        return int(self.blobs[7][0])

    @property
    def max_iter(self):
        return int(self.blobs[7][1])

    @property
    def cell_count(self):
        return int(self.blobs[7][2])

    def nbytes(self):
        return sum(a.nbytes for a in self.blobs.values())


def pick_edit_delta(hit, scene, place, value):
    """tdt_pick_edit_delta: the 8-float DeltaNode {pos, type, value, padding} for a click on the face `hit` found (one record of
    rt.RAY_HIT_DTYPE); place = 1 puts a LEAF of material `value` in the finest cell in front of the face, 0 empties the one
    behind it.  `scene`: a Scene (its slot 6 / 7 payloads) or a (floats[7], ints[3]) pair.  Raises ValueError when the hit
    cannot be edited at (miss, stale record, position outside the octree)."""
    L = lib()
    L.tdt_pick_edit_delta.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    rec = np.ascontiguousarray(np.asarray(hit).reshape(-1)[:1])
    if rec.dtype.itemsize != 64:
        raise TypeError("hit must be a tdt_ray_hit record (rt.RAY_HIT_DTYPE)")
    floats, ints = (scene.blobs[6], scene.blobs[7]) if isinstance(scene, Scene) else scene
    of = np.ascontiguousarray(np.asarray(floats).view(np.float32).reshape(-1)[:7], np.float32)
    oi = np.ascontiguousarray(np.asarray(ints).view(np.int32).reshape(-1)[:3], np.int32)
    out = np.zeros(8, np.float32)
    rc = L.tdt_pick_edit_delta(rec.ctypes.data, of.ctypes.data, oi.ctypes.data, int(place), float(value), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"[{rc:#x}] " + L.tdt_host_last_error().decode())
    return out


def pick_grid_voxel(hit, scene, place):
    """tdt_pick_grid_voxel: the (3,) int32 grid voxel just in front of the face `hit` found (place = 1) or just behind it
    (place = 0) — the cell pick_edit_delta aims at, as a brush centre for rt.Context.octree_edit_region.  Raises ValueError
    when the hit cannot be edited at."""
    L = lib()
    L.tdt_pick_grid_voxel.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    rec = np.ascontiguousarray(np.asarray(hit).reshape(-1)[:1])
    if rec.dtype.itemsize != 64:
        raise TypeError("hit must be a tdt_ray_hit record (rt.RAY_HIT_DTYPE)")
    floats, ints = (scene.blobs[6], scene.blobs[7]) if isinstance(scene, Scene) else scene
    of = np.ascontiguousarray(np.asarray(floats).view(np.float32).reshape(-1)[:7], np.float32)
    oi = np.ascontiguousarray(np.asarray(ints).view(np.int32).reshape(-1)[:3], np.int32)
    out = np.zeros(3, np.int32)
    rc = L.tdt_pick_grid_voxel(rec.ctypes.data, of.ctypes.data, oi.ctypes.data, int(place), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"[{rc:#x}] " + L.tdt_host_last_error().decode())
    return out


def pick_face(hit, scene):
    """tdt_pick_face: (4,) int32 {x, y, z, f} — the grid voxel behind the face `hit` found (pick_grid_voxel with place = 0) and the
    face's direction 0..5 (-x, +x, -y, +y, -z, +z) from the hit normal: a seed for rt.Context.octree_edit_faces.  Raises
    ValueError when the hit cannot be edited at or its normal is not a signed unit axis vector."""
    L = lib()
    L.tdt_pick_face.argtypes = [ctypes.c_void_p] * 4
    rec = np.ascontiguousarray(np.asarray(hit).reshape(-1)[:1])
    if rec.dtype.itemsize != 64:
        raise TypeError("hit must be a tdt_ray_hit record (rt.RAY_HIT_DTYPE)")
    floats, ints = (scene.blobs[6], scene.blobs[7]) if isinstance(scene, Scene) else scene
    of = np.ascontiguousarray(np.asarray(floats).view(np.float32).reshape(-1)[:7], np.float32)
    oi = np.ascontiguousarray(np.asarray(ints).view(np.int32).reshape(-1)[:3], np.int32)
    out = np.zeros(4, np.int32)
    rc = L.tdt_pick_face(rec.ctypes.data, of.ctypes.data, oi.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"[{rc:#x}] " + L.tdt_host_last_error().decode())
    return out


def scene_with_cell_count(scene, cell_count, zero_tail_nodes=0):
    """The same tree as a host with other conventions uploads it: Octree::init_global_buffers writes floats[6] = 1.0 / cell_count as
    f32 and ints[2] = cell_count (octree.rs:49, 79) — the reference's main.rs passes 100000 — and a pre-allocated cells buffer ends in
    zero nodes (main.rs:339-341)."""
    blobs = {k: v.copy() for k, v in scene.blobs.items()}
    blobs[6][6] = np.float32(1.0) / np.float32(cell_count)
    blobs[7][2] = cell_count
    if zero_tail_nodes:
        blobs[0] = np.concatenate([blobs[0], np.zeros(2 * int(zero_tail_nodes), np.uint32)])
    return Scene(blobs, scene.counts, f"{scene.name}_cc{cell_count}" + (f"_tail{zero_tail_nodes}" if zero_tail_nodes else ""))


def _builder(vertical_fov, image_width, aspect_ratio=None, viewport_height=None, origin=None, samples_per_pixel=None,
             max_bounce=None):
    b = CameraBuilderC()
    b.vertical_fov = vertical_fov
    b.image_width = image_width
    if aspect_ratio is not None:
        b.has_aspect_ratio, b.aspect_ratio = 1, aspect_ratio
    if viewport_height is not None:
        b.has_viewport_height, b.viewport_height = 1, viewport_height
    if origin is not None:
        b.has_origin = 1
        b.origin[:] = list(origin)
    if samples_per_pixel is not None:
        b.has_samples_per_pixel, b.samples_per_pixel = 1, samples_per_pixel
    if max_bounce is not None:
        b.has_max_bounce, b.max_bounce = 1, max_bounce
    return b


def camera_build(vertical_fov, image_width, aspect_ratio=None, viewport_height=None, origin=None,
                 samples_per_pixel=None, max_bounce=None):
    """CameraBuilder::new(fov, width).with_*().build() -> the uniforms it uploads (camera.rs:119-253)."""
    b = _builder(vertical_fov, image_width, aspect_ratio, viewport_height, origin, samples_per_pixel, max_bounce)
    u = CameraUniforms()
    _check(lib().tdt_camera_build(ctypes.byref(b), ctypes.byref(u)))
    return u


def camera_reference_pose(width, height, spp, max_bounce):
    """The camera main.rs:165-168 builds, for a width x height window."""
    u = CameraUniforms()
    _check(lib().tdt_camera_reference_pose(width, height, spp, max_bounce, ctypes.byref(u)))
    return u


# ---------------------------------------------------------------- scene ingest ---
def cantor_pair(r, g, b):
    """ply_point_loader.rs:228-241 (f64 arithmetic, saturating `as u32`)."""
    fd = 0.5 * (r + g) * (r + g + 1.0) + g
    h = 0.5 * (fd + b) * (fd + b + 1.0) + b
    return 0xFFFFFFFF if h >= 4294967295.0 else int(h)


class Ply:
    """PlyFileContent of ply_point_loader::from_resources (ply_point_loader.rs:84-93) for a byte buffer."""

    def __init__(self, data, strict_crlf=True):
        L = lib()
        L.tdt_ply_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.tdt_ply_destroy.argtypes = [ctypes.c_void_p]
        L.tdt_ply_destroy.restype = None
        L.tdt_ply_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
        L.tdt_ply_voxels.argtypes = [ctypes.c_void_p]
        L.tdt_ply_voxels.restype = ctypes.POINTER(ctypes.c_int32)
        L.tdt_ply_albedos.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        L.tdt_ply_albedos.restype = ctypes.c_int64
        L.tdt_scene_from_ply.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        h = ctypes.c_void_p()
        _check(L.tdt_ply_parse(bytes(data), len(data), 1 if strict_crlf else 0, ctypes.byref(h)))
        self._h = h
        hv, nv, na = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        mp = (ctypes.c_int32 * 3)()
        _check(L.tdt_ply_info(h, ctypes.byref(hv), ctypes.byref(nv), mp, ctypes.byref(na)))
        self.header_vertex, self.min_point = hv.value, list(mp)
        n = nv.value
        v = np.ctypeslib.as_array(L.tdt_ply_voxels(h), shape=(n, 4)).copy() if n else np.zeros((0, 4), np.int32)
        self.positions = v[:, :3]
        self.albedo_keys = v[:, 3].view(np.uint32) if n else np.zeros(0, np.uint32)
        keys = np.zeros(na.value, np.uint32)
        rgb = np.zeros((na.value, 3), np.uint8)
        L.tdt_ply_albedos(h, keys.ctypes.data, rgb.ctypes.data, na.value)
        self.albedos = {int(k): tuple(int(c) for c in col) for k, col in zip(keys, rgb)}

    def to_scene(self, max_iter=256, z_up=True):
        h = ctypes.c_void_p()
        _check(lib().tdt_scene_from_ply(self._h, max_iter, 1 if z_up else 0, ctypes.byref(h)))
        return Scene._from_handle(h, "ply")

    def __del__(self):
        try:
            if self._h:
                lib().tdt_ply_destroy(self._h)
        except Exception:
            pass


# ---------------------------------------------------------------- triangle meshes ---
def mesh_quantize(xyz, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """tdt_mesh_quantize: (n, 3) float32 vertices -> (n, 3) int32 fixed point, rint((x * scale + offset) * 64) in float64.
    Raises ValueError when a result is not finite or beyond +-2^18 units."""
    L = lib()
    L.tdt_mesh_quantize.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p]
    p = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    out = np.zeros(p.shape, np.int32)
    off = (ctypes.c_double * 3)(*[float(v) for v in offset])
    rc = L.tdt_mesh_quantize(p.ctypes.data if len(p) else None, len(p), float(scale), off, out.ctypes.data if len(p) else None)
    if rc != 0:
        raise ValueError(f"[{rc:#x}] " + L.tdt_host_last_error().decode())
    return out


def mesh_fit(xyz, lo, hi):
    """tdt_mesh_fit: (scale, offset (3,) float64) that centre the vertices' bounding box in the voxel box lo..hi inclusive,
    the limiting edge spanning it."""
    L = lib()
    L.tdt_mesh_fit.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    p = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    scale, off = ctypes.c_double(0), (ctypes.c_double * 3)()
    rc = L.tdt_mesh_fit(p.ctypes.data if len(p) else None, len(p), (ctypes.c_int32 * 3)(*[int(v) for v in lo]),
                        (ctypes.c_int32 * 3)(*[int(v) for v in hi]), ctypes.byref(scale), off)
    if rc != 0:
        raise ValueError(f"[{rc:#x}] " + L.tdt_host_last_error().decode())
    return float(scale.value), np.array(list(off), np.float64)


def quads_to_mesh(quads):
    """tdt_quads_to_mesh: (n, 8) int32 tdt_quad rows (rt.Context.octree_extract_surface) -> (vertices (k, 3) int32 fixed point, 64
    units per voxel, welded and in ascending (x, y, z) order; triangles (2 n, 3) uint32, outward normals; materials (2 n,) int32,
    the quad's material for both of its triangles)."""
    L = lib()
    sz = ctypes.POINTER(ctypes.c_size_t)
    L.tdt_quads_to_mesh.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, sz, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_size_t, sz]
    q = np.asarray(quads)
    if q.size and q.dtype.kind not in "iu":
        raise ValueError(f"quads must be integers, not {q.dtype}")
    q = np.ascontiguousarray(q, np.int32).reshape(-1, 8)
    nv, nt = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(L.tdt_quads_to_mesh(q.ctypes.data if len(q) else None, len(q), None, 0, ctypes.byref(nv), None, None, 0, ctypes.byref(nt)))
    v, t, m = np.zeros((nv.value, 3), np.int32), np.zeros((nt.value, 3), np.uint32), np.zeros(nt.value, np.int32)
    if len(q):
        _check(L.tdt_quads_to_mesh(q.ctypes.data, len(q), v.ctypes.data, len(v), ctypes.byref(nv), t.ctypes.data, m.ctypes.data, len(t),
                                   ctypes.byref(nt)))
    return v, t, m


def ply_mesh_write(vertices, triangles):
    """tdt_ply_mesh_write: a fixed-point mesh ((n, 3) int32 units, (m, 3) vertex indices) as the bytes of an ASCII PLY with
    coordinates in voxels (units / 64, exact), in the grammar PlyMesh reads."""
    L = lib()
    L.tdt_ply_mesh_write.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t)]
    v = np.ascontiguousarray(vertices, np.int32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    pv, pt = (v.ctypes.data if len(v) else None), (t.ctypes.data if len(t) else None)
    n = ctypes.c_size_t(0)
    _check(L.tdt_ply_mesh_write(pv, len(v), pt, len(t), None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(max(n.value, 1))
    _check(L.tdt_ply_mesh_write(pv, len(v), pt, len(t), buf, n.value, ctypes.byref(n)))
    return buf.raw[: n.value]


# ---------------------------------------------------------------- affine transforms ---
def _xform_call(name, argtypes, *args):
    """One tdt_xform_* builder: a fresh rt.Xform filled by the library; ValueError with its message otherwise."""
    from . import rt
    L = lib()
    f = getattr(L, name)
    f.argtypes = list(argtypes) + [ctypes.POINTER(rt.Xform)]
    out = rt.Xform()
    rc = f(*args, ctypes.byref(out))
    if rc != 0:
        raise ValueError(f"[{rc:#x}] " + L.tdt_host_last_error().decode())
    return out


def _i3(name, v):
    v = list(v)
    if len(v) != 3 or any(isinstance(e, (bool, np.bool_)) or int(e) != e or not -2**31 <= int(e) <= 2**31 - 1 for e in v):
        raise ValueError(f"{name} must hold three int32 values, not {v!r}")
    return (ctypes.c_int32 * 3)(*[int(e) for e in v])


def _d(name, v, count):
    v = [float(e) for e in np.asarray(v, np.float64).reshape(-1)]
    if len(v) != count:
        raise ValueError(f"{name} must hold {count} numbers")
    return (ctypes.c_double * count)(*v)


_I3 = ctypes.POINTER(ctypes.c_int32)
_D = ctypes.POINTER(ctypes.c_double)


def xform_identity():
    """tdt_xform_identity: s = p."""
    return _xform_call("tdt_xform_identity", [])


def xform_translate(d):
    """tdt_xform_translate: the selection moves by d = (dx, dy, dz) voxels."""
    return _xform_call("tdt_xform_translate", [_I3], _i3("d", d))


def xform_quarter_turns(axis, k, pivot2):
    """tdt_xform_quarter_turns: k quarter turns about `axis` (0 x, 1 y, 2 z) through pivot2 (doubled coordinates: 2 c + 1 is the
    centre of voxel c); k = 1 about z takes x towards y: numpy.rot90(grid, 1, axes=(0, 1)) when pivot2 = (N, N, N).  A bijection
    of the grid exactly when pivot2's components on the two turned axes have equal parity."""
    return _xform_call("tdt_xform_quarter_turns", [ctypes.c_int, ctypes.c_int, _I3], int(axis), int(k), _i3("pivot2", pivot2))


def xform_mirror(axis, pivot2):
    """tdt_xform_mirror: the reflection of `axis` about the plane through pivot2[axis] (doubled coordinates)."""
    return _xform_call("tdt_xform_mirror", [ctypes.c_int, _I3], int(axis), _i3("pivot2", pivot2))


def xform_scale(num, den, pivot2):
    """tdt_xform_scale: per axis by num / den (integers >= 1) about pivot2 (doubled coordinates)."""
    return _xform_call("tdt_xform_scale", [_I3, _I3, _I3], _i3("num", num), _i3("den", den), _i3("pivot2", pivot2))


def xform_from_affine(fwd):
    """tdt_xform_from_affine: the forward map x' = F x + f on continuous coordinates (voxel c occupies [c, c + 1)) as a (3, 4)
    array [F | f]; inverted and rounded to the struct's fixed point."""
    return _xform_call("tdt_xform_from_affine", [_D], _d("fwd", fwd, 12))


def xform_rotate(axis, degrees, pivot):
    """tdt_xform_rotate: by `degrees` about the line through `pivot` (continuous coordinates; the centre of voxel c is c + 0.5)
    along `axis`."""
    return _xform_call("tdt_xform_rotate", [_D, ctypes.c_double, _D], _d("axis", axis, 3), float(degrees), _d("pivot", pivot, 3))


class PlyMesh:
    """tdt_ply_mesh_parse of a byte buffer: vertices (n, 3) float32, triangles (m, 3) uint32 (polygons fan-triangulated),
    faces = the file's polygon count.  Colours are ignored.  Raises ValueError with the reader's message."""

    def __init__(self, data):
        L = lib()
        L.tdt_ply_mesh_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        L.tdt_ply_mesh_destroy.argtypes = [ctypes.c_void_p]
        L.tdt_ply_mesh_destroy.restype = None
        L.tdt_ply_mesh_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int64)] * 3
        L.tdt_ply_mesh_vertices.argtypes = [ctypes.c_void_p]
        L.tdt_ply_mesh_vertices.restype = ctypes.POINTER(ctypes.c_float)
        L.tdt_ply_mesh_triangles.argtypes = [ctypes.c_void_p]
        L.tdt_ply_mesh_triangles.restype = ctypes.POINTER(ctypes.c_uint32)
        h = ctypes.c_void_p()
        data = bytes(data)
        rc = L.tdt_ply_mesh_parse(data, len(data), ctypes.byref(h))
        if rc != 0:
            raise ValueError(f"[{rc:#x}] " + L.tdt_host_last_error().decode())
        try:
            nv, nf, nt = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            _check(L.tdt_ply_mesh_info(h, ctypes.byref(nv), ctypes.byref(nf), ctypes.byref(nt)))
            self.faces = nf.value
            self.vertices = (np.ctypeslib.as_array(L.tdt_ply_mesh_vertices(h), shape=(nv.value, 3)).copy() if nv.value
                             else np.zeros((0, 3), np.float32))
            self.triangles = (np.ctypeslib.as_array(L.tdt_ply_mesh_triangles(h), shape=(nt.value, 3)).copy() if nt.value
                              else np.zeros((0, 3), np.uint32))
        finally:
            L.tdt_ply_mesh_destroy(h)
