"""Through-selection without a GPU: the entry points are exported and bound, the prototypes are the binding's, the header states
the predicate, tdt_screen_select has its size and offsets, the kernels of tdt_screen.hip cross-compile without scratch or spills and
with no LDS beyond the vertex stage and four counters, the unit and the reprojection call one projection function,
include/renderer.hpp compiles with the new members, the Renderer's existing methods keep their signatures, and the Python calls
refuse bad arguments before anything runs."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tdt4230_project_raytracing_amd import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tdt4230_project_raytracing_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("tdt_octree_extract_screen", "tdt_octree_edit_screen", "tdt_debug_screen_counts")


def _params(f):
    return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]


def test_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    E, inf = inspect.Parameter.empty, float("inf")
    shape = [("rect", None), ("polygon", None), ("mask", None), ("window", False), ("material", None), ("min_distance", 0.0), ("max_distance", inf)]
    assert _params(rt.Context.octree_extract_screen) == [("view", E)] + shape
    assert _params(rt.Context.octree_edit_screen) == [("op", E), ("view", E)] + shape + [("paint_material", 0)]
    assert _params(rt.Context.screen_counts) == []
    sig = inspect.signature(rt.Renderer.select_through)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:4]] == shape[:3]
    assert list(sig.parameters.values())[4].kind is inspect.Parameter.VAR_KEYWORD


def test_prototypes_match_the_binding():
    ctype = {"tdt_ctx *": ctypes.c_void_p, "const tdt_image *": ctypes.c_void_p, "int": ctypes.c_int, "size_t": ctypes.c_size_t,
             "int32_t": ctypes.c_int32, "uint64_t": ctypes.POINTER(ctypes.c_uint64), "const int32_t *": ctypes.c_void_p, "int32_t *": ctypes.c_void_p,
             "size_t *": ctypes.POINTER(ctypes.c_size_t), "uint32_t *": ctypes.POINTER(ctypes.c_uint32),
             "const tdt_view *": ctypes.POINTER(rt.VIEW), "const tdt_screen_select *": ctypes.POINTER(rt.ScreenSelect)}
    protos = {
        "tdt_octree_extract_screen": "tdt_ctx *ctx, const tdt_view *view, const tdt_screen_select *sel, const int32_t *polygon_xy, "
                                     "size_t n_vertices, const tdt_image *mask, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels",
        "tdt_octree_edit_screen": "tdt_ctx *ctx, int op, const tdt_view *view, const tdt_screen_select *sel, const int32_t *polygon_xy, "
                                  "size_t n_vertices, const tdt_image *mask, int32_t material, uint32_t *n_cells",
        "tdt_debug_screen_counts": "tdt_ctx *ctx, uint64_t out[4]",
    }
    bound = {n: (res, args) for n, res, args in rt.SYMBOLS}
    for name, params in protos.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", CODE)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
        types = [re.match(r"(.*?)(\w+)(\[\d+\])?$", p.strip()).group(1).strip() for p in params.split(",")]
        res, args = bound[name]
        assert res is ctypes.c_int and args == [ctype[t] for t in types], name
    # the new block stands after the screen-space selection block
    assert CODE.index("tdt_image_extract_voxels") < CODE.index("tdt_octree_extract_screen") < CODE.index("tdt_octree_census")


def test_the_header_states_the_predicate():
    block = re.search(r"/\* ---- through-selection.*?\*/", HEADER, re.S).group(0)
    text = re.sub(r"\s*\n \*\s*", " ", block)
    for phrase in ("read as tdt_pick_grid_voxel reads them", "u[a] = (2 k[a] + 1) * 2^-(d+1)", "(k[a] + c) * 2^-d with c in {0, 1}", "exact in fp32",
                   "w[a] = (u[a] * scale) + min[a]: two rounded fp32 operations, never fused", "exactly tdt_image_reproject's Q", "D = w - view.origin",
                   "nu = (Ru.z D.z + Ru.y D.y) + Ru.x D.x", "fx = (nu / nw) * (float)(image_width - 1)", "fy = (nv / nw) * (float)(image_height - 1)",
                   "Every operation is rounded, none fused",
                   "nw > 0 && fx >= 0 && fx < (float)image_width && fy >= 0 && fy < (float)image_height", "(px, py) = ((int)fx, (int)fy)",
                   "a NaN (a point at the eye) simply fails", "x0 <= px <= x1 && y0 <= py <= y1", "x0 > x1 or y0 > y1 selects nothing",
                   "P = (2px+1, 2py+1), A = 2a, B = 2b", "closing the last vertex to the first", "(Ay > Py) != (By > Py)",
                   "s = (Px-Ax)*(By-Ay) - (Bx-Ax)*(Py-Ay)", "(By > Ay) ? s < 0 : s > 0", "no vertex lies on the scan line", "the count is odd",
                   "(x0,y0), (x1+1,y0), (x1+1,y1+1), (x0,y1+1)", "exactly image_width x image_height", "mask[py][px].x > 0.0f (NaN and -0 are outside)",
                   "Without TDT_SCREEN_WINDOW the tested point is the centre", "all eight corners must pass", "the centre is not tested",
                   "material < 0 || voxel material == material", "min_distance*min_distance <= dd && dd <= max_distance*max_distance",
                   "dd = (D.z*D.z + D.y*D.y) + D.x*D.x of the centre", "both squares are rounded fp32 products",
                   "An unused polygon_xy or mask is ignored", "follows tdt_octree_extract_region's rules", "SET would equal PAINT and FILL would be empty",
                   "The list never leaves the device", "[0] voxels of V, [1] voxels whose tested points are all in front and on screen",
                   "[3] voxels selected, after material and distance", "a failing call leaves them unchanged", "Before any call all four are 0",
                   "nothing written and nothing queued", "a MASK edit on a multi-device context", "Slots 0, 6 or 7 unbound: TDT_ERR_INCOMPLETE",
                   "No occlusion test", "no hierarchical culling", "a \"crossing\" marquee"):
        assert phrase in text, phrase


def test_struct_size_offsets_and_constants():
    assert len(re.findall(r"sizeof\(tdt_screen_select\) == 36", CODE)) == 2                         # C++ and C
    body = re.search(r"typedef struct tdt_screen_select \{(.*?)\} tdt_screen_select;", CODE, re.S).group(1)
    fields = re.findall(r"\b(float|int32_t|uint32_t)\s+(\w+)(?:\[(\d+)\])?\s*(?:,\s*(\w+))?;", body)
    assert fields == [("int32_t", "shape", "", ""), ("int32_t", "rect", "4", ""), ("uint32_t", "flags", "", ""), ("int32_t", "material", "", ""),
                      ("float", "min_distance", "", "max_distance")]
    S = rt.ScreenSelect
    assert [n for n, _ in S._fields_] == ["shape", "rect", "flags", "material", "min_distance", "max_distance"] and ctypes.sizeof(S) == 36
    assert (S.shape.offset, S.rect.offset, S.flags.offset, S.material.offset, S.min_distance.offset, S.max_distance.offset) == (0, 4, 20, 24, 28, 32)
    m = re.search(r"enum \{ TDT_SCREEN_RECT = (\d+), TDT_SCREEN_POLYGON = (\d+), TDT_SCREEN_MASK = (\d+) \};", CODE)
    assert m and tuple(int(g) for g in m.groups()) == (rt.SCREEN_RECT, rt.SCREEN_POLYGON, rt.SCREEN_MASK) == (0, 1, 2)
    assert int(re.search(r"#define\s+TDT_SCREEN_WINDOW\s+(\d+)u\b", CODE).group(1)) == rt.SCREEN_WINDOW == 1
    assert int(re.search(r"#define\s+TDT_SCREEN_MAX_VERTICES\s+(\d+)\b", CODE).group(1)) == rt.SCREEN_MAX_VERTICES == 256
    # the C struct itself, compiled as C: the offsets are the binding's
    src = "#include <stddef.h>\n#include \"tdt_rt.h\"\n" + "".join(
        "_Static_assert(offsetof(tdt_screen_select, %s) == %d, \"%s\");\n" % (n, getattr(S, n).offset, n) for n, _ in S._fields_)
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_kernels_have_no_scratch_no_spills_and_only_the_vertex_stage_in_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = {re.match(r"tdt::([\w<>]+)", r["name"]).group(1): r for r in kernel_resources.collect("tdt_screen.hip")}
    assert sorted(rows) == ["screen_select_kernel<false>", "screen_select_kernel<true>"]
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, name
        assert r["LDS Size [bytes/block]"] == 256 * 8 + 4 * 4, name                  # 256 doubled vertices of two ints, four counters
    from tdt4230_project_raytracing_amd import build
    assert "tdt_screen.hip" in build.DEVICE_UNITS


def test_the_unit_calls_the_shared_layers_and_q_exists_once():
    text = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".h", ".cpp"))}
    unit = text["tdt_screen.hip"]
    for call in ("view_rows(", "view_project(", "region_edit_selected(", "region_extract_selected(", "query_params(", "first_member(", "device_image(",
                 "blocks_of("):
        assert call in unit, call
    assert "view_project(" in text["reproject_device.hpp"] and "tdt_select" not in unit
    # one definition of the projection and of the per-call rows; the dot products' characteristic line stands nowhere else
    assert [f for f, t in text.items() if re.search(r"TDT_DEV\s+void\s+view_project\(", t)] == ["reproject_device.hpp"]
    assert [f for f, t in text.items() if re.search(r"\bbool view_rows\([^;]*\{", t)] == ["tdt_reproject.hip"]
    found = {f: len(re.findall(r"\(\w+\.?\w*\.rw\[2\] \* dz", t)) for f, t in text.items() if re.search(r"\.rw\[2\] \* dz", t)}
    assert found == {"reproject_device.hpp": 1}, found
    body = re.search(r"TDT_DEV void reproject_body\(.*?\n\}\n", text["reproject_device.hpp"], re.S).group(0)
    assert body.count("view_project(") == 1


def test_renderer_hpp_compiles_with_the_new_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('''#include "renderer.hpp"
using namespace renderer;
uint32_t lasso(Context &ctx, ComputeShader &raytracer, Octree &octree, const Texture &mask) {
  const tdt_view view = raytracer.view();
  tdt_screen_select sel = {TDT_SCREEN_RECT, {10, 10, 40, 30}, TDT_SCREEN_WINDOW, -1, 0.0f, 5.0f};
  const std::vector<int32_t> behind = octree.extract_screen(ctx, view, sel);
  sel.shape = TDT_SCREEN_POLYGON;
  const std::vector<int32_t> polygon = {0, 0, 50, 10, 20, 40};
  const std::vector<int32_t> inside = octree.extract_screen(ctx, view, sel, polygon);
  sel.shape = TDT_SCREEN_MASK;
  const std::vector<int32_t> masked = octree.extract_screen(ctx, view, sel, {}, &mask);
  uint64_t counts[4];
  ctx.check(tdt_debug_screen_counts(ctx.raw(), counts));
  std::vector<int32_t> (Octree::*e)(const Context &, const tdt_view &, const tdt_screen_select &, const std::vector<int32_t> &, const Texture *) const =
      &Octree::extract_screen;
  uint32_t (Octree::*d)(const Context &, int, const tdt_view &, const tdt_screen_select &, const std::vector<int32_t> &, const Texture *, int32_t) const =
      &Octree::edit_screen;
  (void)e; (void)d; (void)behind; (void)inside; (void)masked;
  static_assert(sizeof(tdt_screen_select) == 36 && TDT_SCREEN_MAX_VERTICES == 256, "");
  octree.edit_screen(ctx, TDT_REGION_PAINT, view, sel, {}, &mask, 7);
  sel.shape = TDT_SCREEN_POLYGON;
  return octree.edit_screen(ctx, TDT_REGION_CLEAR, view, sel, polygon, nullptr, 0);
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_existing_render_methods_keep_their_signatures():
    E = inspect.Parameter.empty
    assert _params(rt.Renderer.render) == [("width", None), ("height", None), ("denoise", 0)]
    assert _params(rt.Renderer.render_temporal) == [("width", None), ("height", None), ("cam", None), ("denoise", 0), ("max_samples", 64.0), ("reset", False)]
    assert _params(rt.Renderer.render_upsampled) == [("scale", 2), ("denoise", 0), ("width", None), ("height", None)]
    assert _params(rt.Renderer.render_adaptive) == [("tolerance", E), ("batch", 2), ("min_samples", 4), ("max_samples", None), ("denoise", 0)]
    assert _params(rt.Renderer.render_overlay) == [("voxels", E), ("place", 0), ("fill", (1, .6, 0, .35)), ("edge", (1, .6, 0, 1)), ("edge_width", 1),
                                                   ("voxel_edges", False), ("width", None), ("height", None), ("denoise", 0)]
    assert _params(rt.Renderer.select_rect) == [("rect", E), ("place", 0), ("sample", 0)]
    assert _params(rt.Context.octree_extract_region) == [("regions", E)] and _params(rt.Texture.extract_voxels) == [("rect", None)]


BAD = [dict(), dict(rect=(0, 0, 1, 1), polygon=[(0, 0), (1, 0), (0, 1)]), dict(rect=(0, 0, 1, 1), mask=object()), dict(rect=(0, 0, 1)),
       dict(rect=(0, 0, 1, 1.5)), dict(rect=(0, 0, True, 1)), dict(rect=(0, 0, 1, 2**31)), dict(polygon=[(0, 0), (1, 1)]),
       dict(polygon=[(i, i * i % 7) for i in range(257)]), dict(polygon=[(0, 0), (1, 0), (0, 2**20 + 1)]), dict(polygon=[(0.5, 0), (1, 0), (0, 1)]),
       dict(polygon=[(0, 0, 0), (1, 0, 0), (0, 1, 0)]), dict(mask=np.zeros((4, 4, 4), np.float32)), dict(mask="mask"),
       dict(rect=(0, 0, 1, 1), window=1), dict(rect=(0, 0, 1, 1), material=254), dict(rect=(0, 0, 1, 1), material=-1),
       dict(rect=(0, 0, 1, 1), material=1.0), dict(rect=(0, 0, 1, 1), material=True), dict(rect=(0, 0, 1, 1), min_distance=-1.0),
       dict(rect=(0, 0, 1, 1), min_distance=float("nan")), dict(rect=(0, 0, 1, 1), max_distance=float("nan")),
       dict(rect=(0, 0, 1, 1), min_distance=2.0, max_distance=1.0)]


def test_the_python_calls_refuse_bad_arguments_before_anything_runs():
    class Stub:                                                   # no context, no shader: anything that ran would raise AttributeError
        pass
    view = rt.VIEW()
    for kw in BAD:
        with pytest.raises(ValueError):
            rt.Renderer.select_through(Stub(), **kw)
        with pytest.raises(ValueError):
            rt.Context.octree_extract_screen(Stub(), view, **kw)
        with pytest.raises(ValueError):
            rt.Context.octree_edit_screen(Stub(), rt.REGION_CLEAR, view, **kw)
    with pytest.raises(ValueError):
        rt.Renderer.select_through(Stub(), rect=(0, 0, 1, 1), depth=3)                  # not a filter
    for view in (None, object(), {"image_width": 4}):
        with pytest.raises(ValueError):
            rt.Context.octree_extract_screen(Stub(), view, rect=(0, 0, 1, 1))
        with pytest.raises(ValueError):
            rt.Context.octree_edit_screen(Stub(), rt.REGION_CLEAR, view, rect=(0, 0, 1, 1))
    for m in (-1, 254, 1.0, True, None):
        with pytest.raises(ValueError):
            rt.Context.octree_edit_screen(Stub(), rt.REGION_PAINT, rt.VIEW(), rect=(0, 0, 1, 1), paint_material=m)
    # what is accepted reaches the library: the stub has no handle to give it
    for call in (lambda: rt.Renderer.select_through(Stub(), rect=(0, 0, 1, 1)),
                 lambda: rt.Context.octree_extract_screen(Stub(), rt.VIEW(), polygon=[(0, 0), (4, 0), (0, 4)], window=True, material=0, max_distance=3.0)):
        with pytest.raises(AttributeError):
            call()
