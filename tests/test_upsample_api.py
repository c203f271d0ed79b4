"""Guide-keyed upsampling without a GPU: the entry points are exported and bound, the prototypes are the binding's, upsample_kernel
is the only kernel of tdt_upsample.hip and cross-compiles without scratch or spills and with no LDS beyond its four counters,
include/renderer.hpp compiles with the new member, and Renderer.render and render_temporal keep their signatures."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

from tdt4230_project_raytracing_amd import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tdt_rt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("tdt_image_upsample", "tdt_debug_upsample_counts")


def test_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    assert callable(rt.Texture.upsample) and callable(rt.Context.upsample_counts) and callable(rt.Renderer.render_upsampled)
    assert list(inspect.signature(rt.Texture.upsample).parameters)[1:] == ["dst_guide", "src", "src_guide"]
    sig = inspect.signature(rt.Renderer.render_upsampled)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("scale", 2), ("denoise", 0), ("width", None), ("height", None)]


def test_prototypes_match_the_binding():
    ctype = {"tdt_image *": ctypes.c_void_p, "const tdt_image *": ctypes.c_void_p, "tdt_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32,
             "uint64_t": ctypes.POINTER(ctypes.c_uint64)}
    protos = {
        "tdt_image_upsample": "tdt_image *dst, const tdt_image *dst_guide, const tdt_image *src, const tdt_image *src_guide, uint32_t flags",
        "tdt_debug_upsample_counts": "tdt_ctx *ctx, uint64_t out[4]",
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
    block = re.search(r"/\* ---- guide-keyed upsampling.*?\*/", HEADER, re.S).group(0)
    text = re.sub(r"\s*\n \*\s*", " ", block)
    for phrase in ("A kind-0 texel is treated like any other", "-0 comes back as +0", "SKIPPED unless wt > 0", "read only after the key matched",
                   "bit for bit: class 3", "[1] + [2] + [3] = [0]"):
        assert phrase in text, phrase


def test_kernel_has_no_scratch_no_spills_and_only_its_counters_in_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_upsample.hip")
    assert [re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows] == ["upsample_kernel"]
    r = rows[0]
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0
    assert r["LDS Size [bytes/block]"] == 16                                  # the block's four counters and nothing else
    from tdt4230_project_raytracing_amd import build
    assert "tdt_upsample.hip" in build.DEVICE_UNITS


def test_renderer_hpp_compiles_with_the_new_member(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('''#include "renderer.hpp"
using namespace renderer;
void frame(Context &ctx, ComputeShader &raytracer, Texture &image, const Texture &guide, const Texture &low, const Texture &low_guide, int spp) {
  raytracer.program.set_i32("camera.image_width", low.width());
  raytracer.program.set_i32("camera.image_height", low.height());
  low.bind();
  ctx.check(tdt_dispatch_accumulate(raytracer.program.id(), low.width() + 1, low.height() + 1, 1, 0, spp, nullptr));
  raytracer.dispatch_guide(low_guide);
  raytracer.program.set_i32("camera.image_width", image.width());
  raytracer.program.set_i32("camera.image_height", image.height());
  image.bind();
  raytracer.dispatch_guide(guide);
  image.upsample(guide, low, low_guide);
  image.denoise(guide, 2);
  ctx.check(tdt_dispatch_resolve(raytracer.program.id(), image.width() + 1, image.height() + 1, 1, spp));
  uint64_t counts[4];
  ctx.check(tdt_debug_upsample_counts(ctx.raw(), counts));
  void (Texture::*u)(const Texture &, const Texture &, const Texture &) const = &Texture::upsample;
  (void)u;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_render_upsampled_refuses_a_bad_scale_before_anything_runs():
    class Stub:
        pass
    for bad in (0, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            rt.Renderer.render_upsampled(Stub(), scale=bad)


def test_render_and_render_temporal_keep_their_signatures():
    sig = inspect.signature(rt.Renderer.render)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("self", inspect.Parameter.empty), ("width", None), ("height", None), ("denoise", 0)]
    sig = inspect.signature(rt.Renderer.render_temporal)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("width", None), ("height", None), ("cam", None), ("denoise", 0), ("max_samples", 64.0), ("reset", False)]
