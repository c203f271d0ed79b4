"""The variance unit without a GPU: the three entry points are exported and bound, the prototypes are the binding's, the Python
wrappers and the include/renderer.hpp methods exist and agree with the header, the kernels of tdt_variance.hip cross-compile without
scratch or spills and within the LDS they state, the units share their device code instead of copying it, and the error paths that
need no device answer as the header says."""
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
CSRC = os.path.join(ROOT, "tdt4230_project_raytracing_amd", "csrc")
PROTOS = {
    "tdt_image_variance": "tdt_image *img, const tdt_image *guide, const tdt_image *moments, float min_frames, uint32_t flags",
    "tdt_image_denoise_variance": "tdt_image *img, const tdt_image *guide, int passes, float sigma, float floor, uint32_t flags",
    "tdt_image_reproject_moments": "tdt_compute *c, int sample, const tdt_image *guide, const tdt_image *sums, int spp, "
                                   "const tdt_view *prev_view, const tdt_image *prev_guide, const tdt_image *prev_hist, "
                                   "const tdt_image *prev_moments, float max_samples, tdt_image *hist_out, tdt_image *moments_out, "
                                   "tdt_image *mean_out, uint32_t flags",
}


def test_entry_points_are_exported_and_bound():
    L = ctypes.CDLL(rt.LIB_PATH)
    bound = {n for n, _, _ in rt.SYMBOLS}
    for n in PROTOS:
        assert hasattr(L, n), n
        assert n in bound, n
    sig = inspect.signature(rt.Texture.variance)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("guide", inspect.Parameter.empty), ("moments", None), ("min_frames", 4.0)]
    sig = inspect.signature(rt.Texture.denoise_variance)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("guide", inspect.Parameter.empty), ("passes", inspect.Parameter.empty), ("sigma", inspect.Parameter.empty), ("floor", 0.0)]
    sig = inspect.signature(rt.Texture.reproject_moments)
    assert list(sig.parameters)[1:] == ["shader", "sample", "guide", "spp", "prev", "max_samples", "hist_out", "moments_out", "mean_out"]
    assert sig.parameters["max_samples"].default == 64.0 and sig.parameters["prev"].default is None
    assert rt.VARIANCE_SIGMA == 4.0
    # the renderer's switch is an attribute: render and render_temporal keep the signatures tests/test_reproject_api.py pins
    src = inspect.getsource(rt.Renderer.__init__)
    assert "self.variance = None" in src and "self.variance_min_frames = 4.0" in src
    for fn in (rt.Renderer.render, rt.Renderer.render_temporal):
        body = inspect.getsource(fn)
        assert "self.variance is None" in body or "self.variance is not None" in body, fn.__name__
        assert "denoise_variance(" in body and ".denoise(" in body, fn.__name__


def test_prototypes_match_the_binding():
    V = ctypes.POINTER(rt.VIEW)
    ctype = {"tdt_compute *": ctypes.c_void_p, "tdt_image *": ctypes.c_void_p, "const tdt_image *": ctypes.c_void_p, "int": ctypes.c_int,
             "uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "const tdt_view *": V}
    bound = {n: (res, args) for n, res, args in rt.SYMBOLS}
    for name, params in PROTOS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", CODE)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
        types = [re.match(r"(.*?)(\w+)$", p.strip()).group(1).strip() for p in params.split(",")]
        res, args = bound[name]
        assert res is ctypes.c_int and args == [ctype[t] for t in types], name


def test_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.collect("tdt_variance.hip")
    names = sorted(re.match(r"tdt::(\w+(?:<\d+>)?)", r["name"]).group(1) for r in rows)
    assert names == ["denoise_variance_gather_kernel", "denoise_variance_tile_kernel<1>", "denoise_variance_tile_kernel<2>",
                     "reproject_moments_kernel", "variance_kernel"]
    for r in rows:
        assert r["ScratchSize [bytes/lane]"] == 0, r["name"]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, r["name"]
        lds = r["LDS Size [bytes/block]"]
        if "tile_kernel<1>" in r["name"]:
            assert lds == (32 + 4) * (8 + 4) * 36                      # the tile and a halo of 2: colour + key + luminance
        elif "tile_kernel<2>" in r["name"]:
            assert lds == (32 + 8) * (8 + 8) * 36 < 24 * 1024          # a halo of 4: 640 texels
        elif "variance_kernel" in r["name"] and "denoise" not in r["name"]:
            assert lds == (32 + 6) * (8 + 6) * 20                      # a halo of 3: key + luminance
        elif "reproject_moments_kernel" in r["name"]:
            assert lds == 16                                          # the block's four counters, as reproject_kernel
        else:
            assert lds == 0
    from tdt4230_project_raytracing_amd import build
    assert "tdt_variance.hip" in build.DEVICE_UNITS
    assert "denoise_device.hpp" in build.DEVICE_HEADERS and "reproject_device.hpp" in build.DEVICE_HEADERS


def test_units_share_their_device_code():
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("tdt_denoise.hip", "tdt_variance.hip", "tdt_reproject.hip", "denoise_device.hpp",
                                                            "reproject_device.hpp")}
    for fn in ("key_of", "same_key", "tile_origin", "lum"):
        defined = [f for f, t in text.items() if re.search(r"TDT_DEV\s+\w+\s+" + fn + r"\(", t)]
        assert defined == ["denoise_device.hpp"], (fn, defined)
    for unit in ("tdt_denoise.hip", "tdt_variance.hip"):
        assert '#include "denoise_device.hpp"' in text[unit] and "tile_origin(tiles_x, x0, y0)" in text[unit] and "same_key(" in text[unit], unit
        assert "denoise_sequence(" in text[unit], unit                # one scratch sequence
    assert len(re.findall(r"\bint denoise_sequence\(", text["tdt_denoise.hip"])) == 1 and "hipMalloc" not in text["tdt_variance.hip"]
    # one projection, one FOUND predicate: the body both reprojection kernels instantiate
    assert text["reproject_device.hpp"].count("prev_guide[q]") == 1 and "prev_guide[q]" not in text["tdt_reproject.hip"] + text["tdt_variance.hip"]
    assert "reproject_body<false>(" in text["tdt_reproject.hip"] and "reproject_body<true>(" in text["tdt_variance.hip"]


def test_renderer_hpp_compiles_with_the_new_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('''#include "renderer.hpp"
using namespace renderer;
void frame(Context &ctx, ComputeShader &raytracer, Texture &image, int spp, int k, tdt_view &prev_view, const Texture (&hist)[2],
           const Texture (&guide)[2], const Texture (&moments)[2]) {
  const int cur = k & 1, old = cur ^ 1;
  if (k) image.clear();
  ctx.check(tdt_dispatch_accumulate(raytracer.program.id(), image.width() + 1, image.height() + 1, 1, k * spp, spp, nullptr));
  raytracer.dispatch_guide(guide[cur], k * spp);
  image.reproject_moments(raytracer, k * spp, guide[cur], spp, k ? &prev_view : nullptr, k ? &guide[old] : nullptr, k ? &hist[old] : nullptr,
                          k ? &moments[old] : nullptr, 64.0f, hist[cur], moments[cur], &image);
  image.reproject_moments(raytracer, k * spp, guide[cur], spp, nullptr, nullptr, nullptr, nullptr, 8.0f, hist[cur], moments[cur]);
  image.variance(guide[cur]);
  image.variance(guide[cur], &moments[cur]);
  image.variance(guide[cur], &moments[cur], 2.0f);
  image.denoise_variance(guide[cur], 3, 4.0f);
  image.denoise_variance(guide[cur], 3, 4.0f, 1e-6f);
  ctx.check(tdt_dispatch_resolve(raytracer.program.id(), image.width() + 1, image.height() + 1, 1, 1));
  prev_view = raytracer.view();
  void (Texture::*v)(const Texture &, const Texture *, float) const = &Texture::variance;
  void (Texture::*d)(const Texture &, int, float, float) const = &Texture::denoise_variance;
  void (Texture::*m)(const ComputeShader &, int, const Texture &, int, const tdt_view *, const Texture *, const Texture *, const Texture *, float,
                     const Texture &, const Texture &, const Texture *) const = &Texture::reproject_moments;
  (void)v; (void)d; (void)m;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    demo = open(os.path.join(CSRC, "demo_main.cpp")).read()
    assert '"--variance"' in demo and "denoise_variance(" in demo and "reproject_moments(" in demo


def test_null_handles_are_refused_without_a_device():
    """The checks that come before a context is looked at: a NULL first handle has no context to record a message in, and the call
    returns TDT_ERR_INVALID_VALUE without touching a device."""
    L = rt.lib()
    V = rt.ERR_INVALID_VALUE
    assert L.tdt_image_variance(None, None, None, 4.0, 0) == V
    assert L.tdt_image_denoise_variance(None, None, 1, 1.0, 0.0, 0) == V
    assert L.tdt_image_reproject_moments(None, 0, None, None, 1, None, None, None, None, 64.0, None, None, None, 0) == V
    t = rt.Texture.__new__(rt.Texture)
    try:
        t.reproject_moments(None, 0, None, 4, hist_out=None, moments_out=None)
    except ValueError as e:
        assert "hist_out" in str(e)
    else:
        raise AssertionError("reproject_moments without output textures must raise")
