"""Adaptive sampling without a GPU: the entry points are exported and bound, the prototypes are the binding's, the header states
the contract the numpy model restates, include/renderer.hpp compiles with the new members, the three new kernels cross-compile
without scratch or spills, and the trace kernel's builds are the ones the library held before."""
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
NAMES = ("tdt_dispatch_accumulate_masked", "tdt_image_adapt", "tdt_debug_adapt_counts", "tdt_image_adapt_mean")


def test_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in bound, n
    for f in (rt.ComputeShader.dispatch_accumulate_masked, rt.Texture.adapt, rt.Texture.adapt_mean, rt.Context.adapt_counts,
              rt.Renderer.render_adaptive):
        assert callable(f)
    sig = inspect.signature(rt.ComputeShader.dispatch_accumulate_masked)
    assert list(sig.parameters)[1:] == ["width", "height", "depth", "spp_begin", "spp_count", "carry_ptr", "mask"]
    sig = inspect.signature(rt.Renderer.render_adaptive)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("tolerance", inspect.Parameter.empty), ("batch", 2), ("min_samples", 4), ("max_samples", None), ("denoise", 0)]


def test_prototypes_match_the_binding():
    P = ctypes.c_void_p
    ctype = {"tdt_image *": P, "const tdt_image *": P, "tdt_ctx *": P, "tdt_compute *": P, "void *": P, "uint32_t": ctypes.c_uint32,
             "int": ctypes.c_int, "uint64_t": ctypes.POINTER(ctypes.c_uint64), "const tdt_adapt *": ctypes.POINTER(rt.Adapt)}
    protos = {
        "tdt_dispatch_accumulate_masked": "tdt_compute *c, int width, int height, int depth, int spp_begin, int spp_count, "
                                          "void *carry_device_ptr, const tdt_image *mask",
        "tdt_image_adapt": "const tdt_image *sums, const tdt_image *guide , const tdt_image *state_in, tdt_image *state_out, "
                           "int spp_count, const tdt_adapt *a, uint32_t flags",
        "tdt_debug_adapt_counts": "tdt_ctx *ctx, uint64_t out[4]",
        "tdt_image_adapt_mean": "tdt_image *img, const tdt_image *state, uint32_t flags",
    }
    bound = {n: (res, args) for n, res, args in rt.SYMBOLS}
    for name, params in protos.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", CODE)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
        types = [re.match(r"(.*?)(\w+)(\[\d+\])?$", p.strip()).group(1).strip() for p in params.split(",")]
        res, args = bound[name]
        assert res is ctypes.c_int and args == [ctype[t] for t in types], name
    m = re.search(r"typedef struct tdt_adapt \{(.*?)\} tdt_adapt;", CODE, re.S)
    fields = re.findall(r"(float|int32_t)\s+(\w+);", m.group(1))
    assert fields == [("float", "tolerance"), ("float", "floor"), ("int32_t", "min_samples"), ("int32_t", "max_samples")]
    assert [(n, t) for n, t in rt.Adapt._fields_] == [("tolerance", ctypes.c_float), ("floor", ctypes.c_float),
                                                     ("min_samples", ctypes.c_int32), ("max_samples", ctypes.c_int32)]


def test_the_header_states_the_contract():
    block = re.search(r"/\* ---- adaptive sampling: the sampling controller.*?\*/", HEADER, re.S).group(0)
    text = re.sub(r"\s*\n \*\s*", " ", block)
    for phrase in ("A pixel HAS STOPPED when !(w >= 0.0f)", "lb = (Lc - st.L) / kf", "var = v < 0 ? 0 : v (a NaN stays a NaN)",
                   "P is CAPPED when s' >= hi, and then PASSES", "s' >= lo && n' >= 2.0f && err2 <= thr2", "never from state_out",
                   "state_out[P] = (Lc, m2', n', stopped ? -s' : s')", "[1] + [2] + [3] = [0]", "aw == 0: nothing is written"):
        assert phrase in text, phrase
    masked = re.search(r"/\* tdt_dispatch_accumulate restricted to.*?\*/", HEADER, re.S).group(0)
    text = re.sub(r"\s*\n \*\s*", " ", masked)
    for phrase in ("mask[P].w >= 0.0f: +0 and -0 are live, negative values and NaN are not", "byte for byte", "never a pixel of them"):
        assert phrase in text, phrase


def test_the_controller_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_adaptive.hip")
    names = sorted(re.match(r"tdt::(\w+)", r["name"]).group(1) for r in rows)
    assert names == ["adapt_kernel", "adapt_kernel", "adapt_mean_kernel"]          # adapt_kernel: with and without a guide
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]
    lds = sorted(r["LDS Size [bytes/block]"] for r in rows)
    # the mean: none; without a guide: the four counters; with one: the counters and 34 x 10 keys and tests
    assert lds == [0, 16, 16 + 34 * 10 * (16 + 4)]
    from tdt4230_project_raytracing_amd import build
    assert "tdt_adaptive.hip" in build.DEVICE_UNITS


@pytest.fixture(scope="module")
def trace_unit_rows():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.collect("tdt_rt.hip")


def test_mask_slots_kernel_has_no_scratch_and_no_spills(trace_unit_rows):
    rows = [r for r in trace_unit_rows if r["name"].startswith("tdt::mask_slots_kernel")]
    assert len(rows) == 1
    r = rows[0]
    assert r["ScratchSize [bytes/lane]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0
    assert r["LDS Size [bytes/block]"] == 0


# tdt_debug_trace_variants as the library listed them before masked accumulate: (form, depth, resident, full, brick, unit)
def test_the_trace_builds_are_unchanged():
    rows = rt.trace_variants()
    golden = os.path.join(ROOT, "tests", "golden", "trace_variants.txt")
    want = [tuple(int(v) for v in line.split()) for line in open(golden) if line.strip() and not line.startswith("#")]
    assert rows == want


def test_renderer_hpp_compiles_with_the_new_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('''#include "renderer.hpp"
using namespace renderer;
uint64_t frame(Context &ctx, ComputeShader &raytracer, Texture &image, const Texture &guide, Texture &a, Texture &b, void *carry, int cap) {
  const tdt_adapt limits = {0.05f, 0.05f, 4, cap};
  image.clear(); a.clear();
  Texture *cur = &a, *other = &b;
  uint64_t counts[4] = {0, 0, 0, 0};
  for (int begin = 0;; begin += 2) {
    raytracer.dispatch_accumulate_masked(image.width() + 1, image.height() + 1, 1, begin, 2, carry, *cur);
    if (begin == 0) raytracer.dispatch_guide(guide);
    image.adapt(&guide, *cur, *other, 2, limits);
    Texture *t = cur; cur = other; other = t;
    ctx.check(tdt_debug_adapt_counts(ctx.raw(), counts));
    if (counts[3] == 0) break;
  }
  image.adapt_mean(*cur);
  image.denoise(guide, 2);
  ctx.check(tdt_dispatch_resolve(raytracer.program.id(), image.width() + 1, image.height() + 1, 1, 1));
  void (Texture::*m)(const Texture *, const Texture &, const Texture &, int, const tdt_adapt &) const = &Texture::adapt;
  (void)m;
  image.adapt(nullptr, *cur, *other, 2, limits);
  return counts[0];
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_render_adaptive_refuses_bad_arguments_before_anything_runs():
    class Stub:
        pass
    s = Stub()
    s.camera = Stub()
    s.camera.image_width, s.camera.image_height, s.camera.samples_per_pixel = 8, 8, 4
    s.texture = Stub()
    s.texture.width, s.texture.height = (lambda: 8), (lambda: 8)
    s.ctx = Stub()
    s.ctx.device_count = lambda: 1
    for bad in (0, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            rt.Renderer.render_adaptive(s, 0.05, batch=bad)
    for bad in (0, -3, 8.0, True):
        with pytest.raises(ValueError):
            rt.Renderer.render_adaptive(s, 0.05, max_samples=bad)
    s.ctx.device_count = lambda: 2
    with pytest.raises(ValueError):
        rt.Renderer.render_adaptive(s, 0.05)


def test_existing_renderer_signatures_are_unchanged():
    sig = inspect.signature(rt.Renderer.render)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("self", inspect.Parameter.empty), ("width", None), ("height", None), ("denoise", 0)]
    sig = inspect.signature(rt.ComputeShader.dispatch_accumulate)
    assert list(sig.parameters)[1:] == ["width", "height", "depth", "spp_begin", "spp_count", "carry_ptr"]
