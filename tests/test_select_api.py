"""Screen-space selection without a GPU: the entry points are exported and bound, the prototypes are the binding's, the header
states the contract, the structs have their sizes, the kernels of tdt_select.hip cross-compile without scratch or spills and with
no LDS beyond the staged tile and four counters, include/renderer.hpp compiles with the new members, the Renderer's existing
methods keep their signatures, and render_overlay / select_rect refuse bad arguments before anything runs."""
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
HEADER = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("tdt_dispatch_voxel_ids", "tdt_image_overlay", "tdt_debug_overlay_counts", "tdt_image_extract_voxels")


def test_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    for cls, name in ((rt.ComputeShader, "dispatch_voxel_ids"), (rt.Texture, "read_voxel_ids"), (rt.Texture, "overlay"), (rt.Texture, "extract_voxels"),
                      (rt.Context, "overlay_counts"), (rt.Renderer, "render_overlay"), (rt.Renderer, "select_rect")):
        assert callable(getattr(cls, name)), name

    def params(f):
        return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]
    assert params(rt.ComputeShader.dispatch_voxel_ids) == [("texture", inspect.Parameter.empty), ("place", 0), ("sample", 0)]
    assert params(rt.Texture.overlay) == [("ids", inspect.Parameter.empty), ("voxels", inspect.Parameter.empty), ("fill", inspect.Parameter.empty),
                                          ("edge", None), ("edge_width", 1), ("voxel_edges", False)]
    assert params(rt.Texture.extract_voxels) == [("rect", None)]
    assert params(rt.Renderer.render_overlay) == [("voxels", inspect.Parameter.empty), ("place", 0), ("fill", (1, .6, 0, .35)), ("edge", (1, .6, 0, 1)),
                                                  ("edge_width", 1), ("voxel_edges", False), ("width", None), ("height", None), ("denoise", 0)]
    assert params(rt.Renderer.select_rect) == [("rect", inspect.Parameter.empty), ("place", 0), ("sample", 0)]


def test_prototypes_match_the_binding():
    ctype = {"tdt_image *": ctypes.c_void_p, "const tdt_image *": ctypes.c_void_p, "tdt_ctx *": ctypes.c_void_p, "tdt_compute *": ctypes.c_void_p,
             "int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint64_t": ctypes.POINTER(ctypes.c_uint64), "const int32_t *": ctypes.c_void_p,
             "int32_t *": ctypes.c_void_p, "const int32_t": ctypes.POINTER(ctypes.c_int32), "size_t *": ctypes.POINTER(ctypes.c_size_t),
             "const tdt_overlay *": ctypes.POINTER(rt.Overlay)}
    protos = {
        "tdt_dispatch_voxel_ids": "tdt_compute *c, tdt_image *ids, int place, int sample",
        "tdt_image_overlay": "tdt_image *img, const tdt_image *ids, const int32_t *voxels_xyzm, size_t n, const tdt_overlay *style",
        "tdt_debug_overlay_counts": "tdt_ctx *ctx, uint64_t out[4]",
        "tdt_image_extract_voxels": "const tdt_image *ids, const int32_t rect[4], int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels",
    }
    bound = {n: (res, args) for n, res, args in rt.SYMBOLS}
    for name, params in protos.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", CODE)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
        types = [re.match(r"(.*?)(\w+)(\[\d+\])?$", p.strip()).group(1).strip() for p in params.split(",")]
        res, args = bound[name]
        assert res is ctypes.c_int and args == [ctype[t] for t in types], name


def test_the_header_states_the_contract():
    block = re.search(r"/\* ---- screen-space selection.*?\*/", HEADER, re.S).group(0)
    text = re.sub(r"\s*\n \*\s*", " ", block)
    for phrase in ("exactly as tdt_dispatch_guide traces it", "Reads slots 0, 6 and 7 only",
                   "q = ((double)point[a] - (double)min[a]) / (double)scale + side * (double)normal[a] * half", "half = 0.5 / 2^depth",
                   "k[a] = floor(q * 2^depth)", "0 <= k[a] < 2^depth on all three axes", "the only roundings are the subtraction, the divide and the add",
                   "exactly when tdt_pick_grid_voxel succeeds", "spread3(x) << 2 | spread3(y) << 1 | spread3(z)", "0 when state == 0",
                   "max_depth outside 1..10 (the key must fit 30 bits)", "voxels with a coordinate outside [0, 1024) are dropped",
                   "img is unchanged, bit for bit", "member(P): ids[P].state == 1 and ids[P].key is in the list",
                   "max(|dx|, |dy|) <= edge_width", "ids[Q].state != 1 or ids[Q].key != ids[P].key", "Pixels outside the image are not consulted",
                   "out.c = (in.c * (1.0f - a)) + (col.c * a)", "alpha is in's", "[0] pixels, [1] state == 1 pixels, [2] member pixels, [3] edge pixels",
                   "the last texel in row-major order wins", "material >= 254", "First hit only", "marquee paint or clear is extract followed by edit"):
        assert phrase in text, phrase


def test_struct_sizes_and_fields():
    for name, size in (("tdt_voxel_id_texel", 16), ("tdt_overlay", 40)):
        assert len(re.findall(r"sizeof\(%s\) == %d" % (name, size), CODE)) == 2, name             # C++ and C
    body = re.search(r"typedef struct tdt_voxel_id_texel \{(.*?)\} tdt_voxel_id_texel;", CODE, re.S).group(1)
    assert re.findall(r"\b(uint32_t)\s+(\w+)\s*;", body) == [("uint32_t", n) for n in ("state", "key", "material", "t")]
    assert rt.VOXEL_ID_TEXEL_DTYPE.names == ("state", "key", "material", "t") and rt.VOXEL_ID_TEXEL_DTYPE.itemsize == 16
    body = re.search(r"typedef struct tdt_overlay \{(.*?)\} tdt_overlay;", CODE, re.S).group(1)
    fields = re.findall(r"\b(float|int32_t|uint32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert fields == [("float", "fill", "4"), ("float", "edge", "4"), ("int32_t", "edge_width", ""), ("uint32_t", "flags", "")]
    assert [n for n, _ in rt.Overlay._fields_] == [f[1] for f in fields] and ctypes.sizeof(rt.Overlay) == 40
    assert rt.Overlay.edge.offset == 16 and rt.Overlay.edge_width.offset == 32 and rt.Overlay.flags.offset == 36
    m = re.search(r"#define\s+TDT_OVERLAY_VOXEL_EDGES\s+(\d+)u?\b", CODE)
    assert m and int(m.group(1)) == rt.OVERLAY_VOXEL_EDGES == 1


def test_kernels_have_no_scratch_no_spills_and_only_the_staged_tile_in_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = {re.match(r"tdt::([\w<>]+)", r["name"]).group(1): r for r in kernel_resources.collect("tdt_select.hip")}
    own = ["voxel_ids_kernel", "overlay_list_keys_kernel", "rect_pairs_kernel"] + ["overlay_kernel<%d>" % ew for ew in range(5)]
    shared = ["scan_tiles_kernel", "scan_add_kernel"]                         # device_scan.hpp's, instantiated by every unit that scans
    assert sorted(rows) == sorted(own + shared)
    for name in own:
        r = rows[name]
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, name
    assert rows["voxel_ids_kernel"]["LDS Size [bytes/block]"] == 2            # fetch_node's escape entry, as guide_kernel
    assert rows["overlay_list_keys_kernel"]["LDS Size [bytes/block]"] == 0 and rows["rect_pairs_kernel"]["LDS Size [bytes/block]"] == 0
    for ew in range(5):                                                       # (32 + 2 ew) x (8 + 2 ew) texels of key (16 B) and flags (4 B), four counters
        texels = (32 + 2 * ew) * (8 + 2 * ew)
        assert texels <= 40 * 16
        assert rows["overlay_kernel<%d>" % ew]["LDS Size [bytes/block]"] == texels * 20 + 16, ew
    from tdt4230_project_raytracing_amd import build
    assert "tdt_select.hip" in build.DEVICE_UNITS


def test_the_unit_calls_the_shared_layers():
    text = open(os.path.join(ROOT, "tdt4230_project_raytracing_amd", "csrc", "tdt_select.hip")).read()
    for call in ("ray_tile_pixel(", "tile_origin(", "stage_tile<EW>(", "image_grid(", "images_of_context(", "images_fit(", "camera_program(",
                 "device_image(", "query_params(", "query_camera(", "query_first_hit(", "region_key(", "lower_bound_u32(", "voxlist_last_flags(",
                 "voxlist_unique(", "sort_pairs_u32(", "list_to_host(", "first_member("):
        assert call in text, call


def test_renderer_hpp_compiles_with_the_new_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('''#include "renderer.hpp"
using namespace renderer;
uint32_t marquee(Context &ctx, ComputeShader &raytracer, Octree &octree, Texture &image, const Texture &ids, const std::vector<int32_t> &preview) {
  raytracer.dispatch_voxel_ids(ids);
  raytracer.dispatch_voxel_ids(ids, 1, 3);
  const tdt_overlay style = {{1.0f, 0.6f, 0.0f, 0.35f}, {1.0f, 0.6f, 0.0f, 1.0f}, 1, TDT_OVERLAY_VOXEL_EDGES};
  image.overlay(ids, preview, style);
  uint64_t counts[4];
  ctx.check(tdt_debug_overlay_counts(ctx.raw(), counts));
  const int32_t rect[4] = {10, 10, 40, 30};
  const std::vector<int32_t> all = ids.extract_voxels(), some = ids.extract_voxels(rect);
  void (ComputeShader::*d)(const Texture &, int, int) const = &ComputeShader::dispatch_voxel_ids;
  void (Texture::*o)(const Texture &, const std::vector<int32_t> &, const tdt_overlay &) const = &Texture::overlay;
  std::vector<int32_t> (Texture::*e)(const int32_t *) const = &Texture::extract_voxels;
  (void)d; (void)o; (void)e; (void)all;
  static_assert(sizeof(tdt_voxel_id_texel) == 16 && sizeof(tdt_overlay) == 40, "");
  return octree.edit_voxels(ctx, TDT_REGION_CLEAR, some);
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_existing_render_methods_keep_their_signatures():
    E = inspect.Parameter.empty

    def params(f):
        return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]
    assert params(rt.Renderer.render) == [("width", None), ("height", None), ("denoise", 0)]
    assert params(rt.Renderer.render_temporal) == [("width", None), ("height", None), ("cam", None), ("denoise", 0), ("max_samples", 64.0), ("reset", False)]
    assert params(rt.Renderer.render_upsampled) == [("scale", 2), ("denoise", 0), ("width", None), ("height", None)]
    assert params(rt.Renderer.render_adaptive) == [("tolerance", E), ("batch", 2), ("min_samples", 4), ("max_samples", None), ("denoise", 0)]


def test_render_overlay_and_select_rect_refuse_bad_arguments_before_anything_runs():
    class Stub:
        pass
    none = np.zeros((0, 4), np.int32)
    for kw in (dict(place=2), dict(place=-1), dict(place=True), dict(place=None), dict(edge_width=5), dict(edge_width=-1), dict(edge_width=1.0),
               dict(edge_width=True), dict(fill=(1, 0, 0)), dict(edge=(1, 0, 0, 1, 1)), dict(fill="red")):
        with pytest.raises(ValueError):
            rt.Renderer.render_overlay(Stub(), none, **kw)
    with pytest.raises(ValueError):
        rt.Renderer.render_overlay(Stub(), np.zeros((2, 3), np.int32))         # not a list of {x, y, z, m}
    for rect in (None, (0, 0, 1), (0, 0, 1, 1, 1), (0, 0, 1.5, 2), (0, 0, True, 2)):
        with pytest.raises(ValueError):
            rt.Renderer.select_rect(Stub(), rect)
    for kw in (dict(place=2), dict(place=None), dict(sample=-1), dict(sample=0.0), dict(sample=True)):
        with pytest.raises(ValueError):
            rt.Renderer.select_rect(Stub(), (0, 0, 1, 1), **kw)
