"""Cameras whose primary rays are exactly degenerate, and the premises a test of them checks on the CPU.  Plain numpy: no torch.

The shader forms a primary ray as dir = (horizontal * u + lower_left_corner) + (v * vertical - origin), component by component
(raytracer.comp:304-307 as compiled), and normalises it.  A pinhole camera's jittered rays never have a component that is exactly
zero; these uniforms give one to every pixel and sample, whatever the jitter:

  plane bundle   one of horizontal / vertical is the zero vector, the other frame vectors have no component on `axis`, and
                 lower_left_corner[axis] == origin[axis]: d_axis = x + (-x) = +0, its reciprocal +inf
  line           horizontal and vertical both zero: every ray is origin + t * direction
  -0             d_axis = -0 (reciprocal -inf).  Round-to-nearest gives x + (-x) = +0 for every x, and -0 only as (-0) + (-0): so the
                 zero components of horizontal and vertical are -0, lower_left_corner[axis] is -0 and origin[axis] is +0.  The bundle
                 then lies in the plane w_axis = 0, and a test that wants that plane to be a cell face inside the octree places the
                 octree accordingly (corner component -k / 2^depth)
  tiny, denormal the zeroed frame vector has 2^-120 (outside q_rcp3's exponent window) or 2^-140 (a denormal; its reciprocal
                 overflows to +inf) on `axis`.  Any larger |origin[axis]| absorbs such a term, so these too have origin[axis] == +0

A ray lying in the plane of a cell face meets 0 * inf = NaN as a slab operand of every LEAF whose lower face is that plane: the
lookup of a point on the plane lands in the cell above it, whose corner is computed as fl(fl(k / 2^depth * scale) + min)
(face_coordinate) — equal to origin[axis] bit for bit.  An odd k makes the plane a face of finest-level cells only."""
import numpy as np

from tdt4230_project_raytracing_amd import host

F = np.float32
W, H, SPP, BOUNCE = 96, 64, 3, 6
TINY = F(2.0) ** F(-120)
DENORMAL = F(2.0) ** F(-140)
MOVE = F(3e-5)                                # the premise's sidestep: off the face, the view all but unchanged
_VECTORS = ("horizontal", "vertical", "lower_left_corner", "origin")


def is_neg_zero(x):
    return F(x) == 0 and bool(np.signbit(F(x)))


def face_coordinate(k, depth, scale=1.0, min_c=-0.5):
    """World coordinate of grid plane k of 2^depth as the traversal computes a cell's corner (raytracer.comp:427, 441):
    g = sum of bits * 2^-level = k / 2^depth exactly, then fl(fl(g * scale) + min)."""
    g = F(k) / F(1 << depth)
    assert float(g) * (1 << depth) == k
    return F(F(g * F(scale)) + F(min_c))


def _uniforms(hor, ver, llc, origin, w, h, spp, bounce):
    u = host.CameraUniforms()
    u.image_width, u.image_height, u.samples_per_pixel, u.max_bounce = w, h, spp, bounce
    for name, v in zip(_VECTORS, (hor, ver, llc, origin)):
        getattr(u, name)[:] = [float(x) for x in np.asarray(v, F)]
    return u


def camera_bits(u):
    """The twelve float uniforms as raw uint32 bits (-0 and denormals survive), in _VECTORS order."""
    return np.array([list(getattr(u, n)) for n in _VECTORS], F).reshape(-1).view(np.uint32).copy()


def camera_from_bits(bits, w=W, h=H, spp=SPP, bounce=BOUNCE):
    v = np.asarray(bits, np.uint32).view(F).reshape(4, 3)
    return _uniforms(v[0], v[1], v[2], v[3], w, h, spp, bounce)


def _signed_zeros(v, zero):
    v = np.asarray(v, F).copy()
    v[v == 0] = zero
    return v


def plane_bundle(axis, origin, view=(0.0, 0.0, -1.0), fov=90.0, neg_zero=False, axis_component=0.0, w=W, h=H, spp=SPP, bounce=BOUNCE):
    """Every primary ray lies in the plane w[axis] = origin[axis].  `view`: an axis direction other than +-y and other than `axis`.
    The frame is the usual one (right = view x up, up = right x view); the frame vector along `axis` is the one made zero, so a
    y bundle sweeps the image's columns and an x or z bundle its rows.  float32 throughout."""
    o = np.asarray(origin, F)
    d = np.asarray(view, F)
    assert sorted(np.abs(d).tolist()) == [0.0, 0.0, 1.0] and d[axis] == 0 and d[1] == 0
    right = np.cross(d, np.array([0, 1, 0], F)).astype(F)
    up = np.cross(right, d).astype(F)
    vh = F(2.0 * np.tan(np.radians(fov) / 2.0))
    vw = F(F(w) / F(h)) * vh
    hor, ver = (right * vw).astype(F), (up * vh).astype(F)
    zeroed = [v for v in (hor, ver) if v[axis] != 0]
    assert len(zeroed) == 1, "exactly one frame vector lies along the axis"
    zeroed[0][:] = 0
    llc = (o - hor * F(0.5) - ver * F(0.5) + d).astype(F)
    zero = F(-0.0) if neg_zero else F(0.0)
    hor, ver = _signed_zeros(hor, zero), _signed_zeros(ver, zero)
    if neg_zero or axis_component != 0:
        assert o[axis] == 0 and not np.signbit(o[axis]), "d_axis = -0 or a tiny d_axis needs origin[axis] == +0"
        llc[axis] = zero
        zeroed = hor if not np.any(hor != 0) else ver
        zeroed[axis] = F(axis_component) if axis_component != 0 else zero
    else:
        llc[axis] = o[axis]
    return _uniforms(hor, ver, llc, o, w, h, spp, bounce)


def line(origin, direction, w=W, h=H, spp=SPP, bounce=BOUNCE):
    """Every primary ray is origin + t * normalize(direction).  A component of `direction` given as -0.0 comes out as -0 (needs
    origin == +0 there); a +0 component needs lower_left_corner == origin there."""
    o = np.asarray(origin, F)
    d = np.asarray(direction, F)
    llc = (o + d).astype(F)
    hor, ver = np.zeros(3, F), np.zeros(3, F)
    for i in range(3):
        if d[i] == 0:
            llc[i] = o[i]
            if np.signbit(d[i]):
                assert o[i] == 0 and not np.signbit(o[i]), "d = -0 needs origin == +0 on that axis"
                llc[i] = hor[i] = ver[i] = F(-0.0)
        else:
            assert F(llc[i] + -o[i]) == d[i], "choose origin and direction so that (origin + d) - origin == d exactly"
    return _uniforms(hor, ver, llc, o, w, h, spp, bounce)


def moved(cam, axis, by=MOVE):
    """The same camera `by` further along `axis` (origin and lower_left_corner alike: the bundle stays a bundle, off the face)."""
    c = cam.copy()
    new = F(F(cam.origin[axis]) + by)
    assert new != F(cam.origin[axis])
    c.origin[axis] = float(new)
    c.lower_left_corner[axis] = float(new)
    return c


def axis_component_bits(cam, axis):
    """The distinct bit patterns of the unnormalised d[axis] over the (u, v) range a frame uses.  Normalising multiplies by a
    positive finite number, which keeps a zero and its sign."""
    hx, vx, lx, ox = (F(getattr(cam, n)[axis]) for n in _VECTORS)
    t = np.array([0.0, 2.0 ** -24, 0.25, 0.5, 1.0, 1.0 + 1.0 / (min(cam.image_width, cam.image_height) - 1)], F)
    u, v = np.meshgrid(t, t)
    with np.errstate(under="ignore"):
        d = ((hx * u + lx) + (v * vx + -ox)).astype(F)
    return sorted(set(d.view(np.uint32).ravel().tolist()))


def differ(a, b):
    """Share of pixels that differ in any bit."""
    return float((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).mean())


def empty_tree(scene):
    return host.Scene({**scene.blobs, 0: np.zeros(16, np.uint32)}, None, "empty")


NAN_TESTS, VIEW_SHARE = 1000, 0.2


def premises(oracle, scene, cam, axis, kind, nan_tests=NAN_TESTS, threads=8):
    """Checks, with the oracle alone, that the case is what it claims; returns (oracle image, its stats, smallest view share).
    kind "nan": at least `nan_tests` slab tests of the frame have a NaN operand, the tree is in view (a fifth of the pixels differ
    from an all-EMPTY tree's), the NaNs are the face's doing (MOVE further along the axis there is none) and matter (a fifth of
    the pixels differ from that frame).  kind "inf": +-inf operands but no NaN, and the tree in view.  kind "view": the tree in view and +-inf operands
    (a case whose claim is about the direction's bits, which its test checks itself)."""
    ref, st = oracle.render(scene, cam, threads=threads, want_stats=True)
    assert kind in ("nan", "inf", "view")
    share = differ(ref, oracle.render(empty_tree(scene), cam, threads=threads))
    assert share >= VIEW_SHARE, f"the tree is not in view: {share:.3f} of the pixels differ from an empty tree's"
    assert st["inf_slab_tests"] > 0
    if kind == "inf":
        assert st["nan_slab_tests"] == 0, st["nan_slab_tests"]
    if kind == "nan":
        assert st["nan_slab_tests"] >= nan_tests, f"{st['nan_slab_tests']} slab tests with a NaN operand, {nan_tests} wanted"
        off, st_off = oracle.render(scene, moved(cam, axis), threads=threads, want_stats=True)
        assert st_off["nan_slab_tests"] == 0, st_off["nan_slab_tests"]
        near = differ(ref, off)
        assert near >= VIEW_SHARE, f"only {near:.3f} of the pixels differ from the camera moved off the face"
        share = min(share, near)
    return ref, st, share


# ---- the fixture cases (tests/golden/degenerate/*.npz, made by oracle/make_goldens.py --degenerate) -------------------------
HASH6 = ("generate", host.SCENE_HASH_GRID, 6, 1 << 16, 100, 7)
TERRAIN7 = ("generate", host.SCENE_TERRAIN, 7, 1 << 16, 256, 7)
K6 = (1 << 6) // 2 - 5                        # 27: odd, so the plane is a face of finest-level cells only


def _k(depth):
    return (1 << depth) // 2 - 5


def _fc(depth, min_c=-0.5):
    return face_coordinate(_k(depth), depth, 1.0, min_c)


# name -> (scene spec, octree corner or None for the scene's own (-0.5, -0.5, -1), axis, kind, camera)
# kind: the premises the case must meet (see premises()); "view" = the tree in view only.  The cameras stand at the reference pose
# (0.5, 0.4, 0.7) from the corner, looking along -z, with the axis coordinate put on the face.
FIXTURES = {
    "config2_yplane": (("config", 2), None, 1, "nan", lambda: plane_bundle(1, (0.0, _fc(6), -0.3))),
    "config2_xplane": (("config", 2), None, 0, "nan", lambda: plane_bundle(0, (_fc(6), -0.1, -0.3))),
    "config2_yplane_outside": (("config", 2), None, 1, "nan", lambda: plane_bundle(1, (0.0, _fc(6), 0.6), fov=60.0)),
    "config2_yplane_off_face": (("config", 2), None, 1, "inf", lambda: plane_bundle(1, (0.0, -0.1, -0.3))),
    # 16 spp: two-phase frames (a probe launch, then the rest in cost order).  The miss pre-pass runs for cameras outside the octree
    # only, so the frame that goes through both stands at the outside pose
    "config2_yplane_spp16": (("config", 2), None, 1, "nan", lambda: plane_bundle(1, (0.0, _fc(6), -0.3), spp=16)),
    "config2_yplane_outside_spp16": (("config", 2), None, 1, "nan", lambda: plane_bundle(1, (0.0, _fc(6), 0.6), fov=60.0, spp=16)),
    # d_y = -0, 2^-120 * v, 2^-140 * v: the octree placed so that its face plane k = 27 is y = 0 (see the module text)
    "config2_y0_negzero": (("config", 2), (-0.5, -K6 / 64, -1.0), 1, "nan", lambda: plane_bundle(1, (0.0, 0.0, -0.3), neg_zero=True)),
    "config2_y0_tiny": (("config", 2), (-0.5, -K6 / 64, -1.0), 1, "view", lambda: plane_bundle(1, (0.0, 0.0, -0.3), axis_component=TINY)),
    "config2_y0_denormal": (("config", 2), (-0.5, -K6 / 64, -1.0), 1, "nan", lambda: plane_bundle(1, (0.0, 0.0, -0.3), axis_component=DENORMAL)),
    "hash6_xplane": (HASH6, None, 0, "nan", lambda: plane_bundle(0, (_fc(6), -0.1, -0.3))),
    "terrain7_yplane": (TERRAIN7, None, 1, "nan", lambda: plane_bundle(1, (0.0, _fc(7), -0.3))),
    "config3_xplane": (("config", 3), None, 0, "nan", lambda: plane_bundle(0, (_fc(8), -0.1, -0.3))),
    "config5_yplane": (("config", 5), None, 1, "nan", lambda: plane_bundle(1, (0.0, _fc(9), -0.3))),        # 3 spp: llvmpipe loses samples on deep scenes above ~4
    "config2_corner0_yplane": (("config", 2), (0.0, 0.0, 0.0), 1, "nan", lambda: plane_bundle(1, (0.5, _fc(6, 0.0), 0.7))),
    # rays lying in the octree's min face x = 0 itself, origin.x = +0 and -0: w_x - min_x is 0 at the root test too (0 * inf there)
    "config2_corner0_minface_pos": (("config", 2), (0.0, 0.0, 0.0), 0, "nan", lambda: plane_bundle(0, (0.0, 0.4, 0.7))),
    "config2_corner0_minface_neg": (("config", 2), (0.0, 0.0, 0.0), 0, "nan", lambda: plane_bundle(0, (F(-0.0), 0.4, 0.7))),
}


def fixture_scene(spec, corner):
    scene = host.Scene.config(spec[1]) if spec[0] == "config" else host.Scene.generate(*spec[1:])
    if corner is not None:
        blobs = {k: v.copy() for k, v in scene.blobs.items()}
        blobs[6][:3] = np.asarray(corner, F)
        scene = host.Scene(blobs, scene.counts, scene.name + "_placed")
    return scene


def outside(scene, cam):
    """Whether the camera stands outside the octree, as the library decides it before a frame (then the miss pre-pass runs)."""
    f = scene.blobs[6]
    return any(F(cam.origin[a]) < f[a] or F(cam.origin[a]) > F(f[a] + f[4]) for a in range(3))


def fixture_case(name):
    """(scene, camera, axis, kind) of a fixture, built from its parameters."""
    spec, corner, axis, kind, cam = FIXTURES[name]
    return fixture_scene(spec, corner), cam(), axis, kind
