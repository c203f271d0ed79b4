"""Temporal reprojection without a GPU: the entry points are exported and bound, the prototypes are the binding's, tdt_view is 56
bytes field for field in C and in Python, the two kernels of tdt_reproject.hip cross-compile without scratch or spills and with no
LDS beyond their four counters, include/renderer.hpp compiles with the new members, and Renderer.render is what it was."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

from tdt4230_project_raytracing_amd import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("tdt_compute_view", "tdt_image_reproject", "tdt_debug_reproject_counts", "tdt_image_clear")


def test_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    assert callable(rt.ComputeShader.view) and callable(rt.Texture.reproject) and callable(rt.Texture.clear)
    assert callable(rt.Context.reproject_counts) and callable(rt.Renderer.render_temporal)
    sig = inspect.signature(rt.Renderer.render_temporal)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("width", None), ("height", None), ("cam", None), ("denoise", 0), ("max_samples", 64.0), ("reset", False)]
    sig = inspect.signature(rt.Texture.reproject)
    assert list(sig.parameters)[1:] == ["shader", "sample", "guide", "spp", "prev", "max_samples", "hist_out", "mean_out"]
    assert sig.parameters["max_samples"].default == 64.0 and sig.parameters["prev"].default is None


def test_prototypes_match_the_binding():
    V = ctypes.POINTER(rt.VIEW)
    ctype = {"tdt_compute *": ctypes.c_void_p, "const tdt_compute *": ctypes.c_void_p, "tdt_image *": ctypes.c_void_p,
             "const tdt_image *": ctypes.c_void_p, "tdt_ctx *": ctypes.c_void_p, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32,
             "float": ctypes.c_float, "tdt_view *": V, "const tdt_view *": V, "uint64_t": ctypes.POINTER(ctypes.c_uint64)}
    protos = {
        "tdt_compute_view": "const tdt_compute *c, tdt_view *out",
        "tdt_image_reproject": "tdt_compute *c, int sample, const tdt_image *guide, const tdt_image *sums, int spp, "
                               "const tdt_view *prev_view, const tdt_image *prev_guide, const tdt_image *prev_hist, "
                               "float max_samples, tdt_image *hist_out, tdt_image *mean_out, uint32_t flags",
        "tdt_debug_reproject_counts": "tdt_ctx *ctx, uint64_t out[4]",
        "tdt_image_clear": "tdt_image *img",
    }
    bound = {n: (res, args) for n, res, args in rt.SYMBOLS}
    for name, params in protos.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", CODE)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
        types = [re.match(r"(.*?)(\w+)(\[\d+\])?$", p.strip()).group(1).strip() for p in params.split(",")]
        res, args = bound[name]
        assert res is ctypes.c_int and args == [ctype[t] for t in types], name


def test_view_is_56_bytes_field_for_field(tmp_path):
    body = re.search(r"typedef struct tdt_view \{(.*?)\} tdt_view;", CODE, re.S).group(1)
    fields = []
    for typ, names in re.findall(r"\b(float|int32_t)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), typ, int(m.group(2) or 1)))
    assert fields == [("origin", "float", 3), ("lower_left_corner", "float", 3), ("horizontal", "float", 3), ("vertical", "float", 3),
                      ("image_width", "int32_t", 1), ("image_height", "int32_t", 1)]
    want = {"float": ctypes.c_float, "int32_t": ctypes.c_int32}
    off = 0
    assert [f[0] for f in rt.VIEW._fields_] == [f[0] for f in fields]
    for (name, typ, n), (pname, ptype) in zip(fields, rt.VIEW._fields_):
        assert ptype is (want[typ] * n if n > 1 else want[typ]), name
        assert getattr(rt.VIEW, pname).offset == off, name
        off += 4 * n
    assert off == ctypes.sizeof(rt.VIEW) == 56
    assert len(re.findall(r"sizeof\(tdt_view\) == 56", CODE)) == 2            # C++ and C
    src = tmp_path / "view.c"                                                 # and the C compiler agrees, offsets included
    src.write_text('#include <stddef.h>\n#include "tdt_rt.h"\n'
                   '_Static_assert(offsetof(tdt_view, lower_left_corner) == 12 && offsetof(tdt_view, horizontal) == 24 && '
                   'offsetof(tdt_view, vertical) == 36 && offsetof(tdt_view, image_width) == 48 && offsetof(tdt_view, image_height) == 52, "");\n')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_kernel_has_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_reproject.hip")
    assert sorted(re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows) == ["reproject_kernel", "reproject_moments_kernel"]
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]
        assert r["LDS Size [bytes/block]"] == 16, r["name"]                    # the block's four counters and nothing else
    from tdt4230_project_raytracing_amd import build
    assert "tdt_reproject.hip" in build.DEVICE_UNITS


def test_renderer_hpp_compiles_with_the_new_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('''#include "renderer.hpp"
using namespace renderer;
void frame(Context &ctx, ComputeShader &raytracer, Texture &image, int spp, int k, tdt_view &prev_view, const Texture (&hist)[2],
           const Texture (&guide)[2]) {
  const int cur = k & 1, old = cur ^ 1;
  if (k) image.clear();
  ctx.check(tdt_dispatch_accumulate(raytracer.program.id(), image.width() + 1, image.height() + 1, 1, k * spp, spp, nullptr));
  raytracer.dispatch_guide(guide[cur], k * spp);
  image.reproject(raytracer, k * spp, guide[cur], spp, k ? &prev_view : nullptr, k ? &guide[old] : nullptr, k ? &hist[old] : nullptr, 64.0f,
                  hist[cur], &image);
  image.reproject(raytracer, k * spp, guide[cur], spp, nullptr, nullptr, nullptr, 8.0f, hist[cur]);
  ctx.check(tdt_dispatch_resolve(raytracer.program.id(), image.width() + 1, image.height() + 1, 1, 1));
  prev_view = raytracer.view();
  static_assert(sizeof(prev_view) == 56, "");
  uint64_t counts[4];
  ctx.check(tdt_debug_reproject_counts(ctx.raw(), counts));
  tdt_view (ComputeShader::*v)() const = &ComputeShader::view;
  void (Texture::*c)() const = &Texture::clear;
  (void)v; (void)c;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_render_keeps_its_signature():
    sig = inspect.signature(rt.Renderer.render)
    assert [(p.name, p.default, p.kind) for p in sig.parameters.values()] == [
        ("self", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("width", None, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("height", None, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("denoise", 0, inspect.Parameter.POSITIONAL_OR_KEYWORD)]
    assert rt.Renderer.render.__defaults__ == (None, None, 0)
