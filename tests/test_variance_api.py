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
                     "variance_kernel"]                            # (reproject_moments_kernel: tests/test_reproject_api.py)
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
        else:
            assert lds == 0
    from tdt4230_project_raytracing_amd import build
    assert "tdt_variance.hip" in build.DEVICE_UNITS
    assert "denoise_device.hpp" in build.DEVICE_HEADERS and "reproject_device.hpp" in build.DEVICE_HEADERS


# what is matched is the DEFINITION (its characteristic line), not the name: a copy under another name is found too
ONE_DEFINITION = {
    "the B3 table": (r"\{0\.0625f, 0\.25f, 0\.375f, 0\.25f, 0\.0625f\}", "denoise_device.hpp"),
    "the prefilter table": (r"\{0\.25f, 0\.5f, 0\.25f\}", "denoise_device.hpp"),
    "the variance-guided weight's cut": (r"\bd2 < lim\)", "denoise_device.hpp"),
    "the usable limit": (r"lim > 0\.f && lim < INFINITY", "denoise_device.hpp"),
    "the staging loop's bounds test": (r"gx >= 0 && gx < w && gy >= 0 && gy < h", "denoise_device.hpp"),
    "the 16x16 tile's pixel": (r"threadIdx\.x & \(k\w+ - 1\)\)\)[;,] y = ", "denoise_device.hpp"),
    "the 32x8 tile's origin": (r"x0 = \(int\)tx \* kTileW", "denoise_device.hpp"),
    "the too-large refusal": (r"> 0x7FFFFFFFull\) return (tdt::)?fail\(", "tdt_internal.hpp"),
    "the first-member camera": (r"replicas\.empty\(\) \? c : c->replicas\[0\]", "tdt_internal.hpp"),
    "the N-handle overlap loop": (r"== \w+\[j\] \|\| (tdt::)?overlap\(", "tdt_internal.hpp"),
    "the reprojection's history read": (r"prev_guide\[q\]", "reproject_device.hpp"),
    "the scratch sequence": (r"\bint denoise_sequence\([^;]*\{", "tdt_denoise.hip"),
    "the scratch sequence's caller": (r"(?<!int )\bdenoise_sequence\(", "tdt_internal.hpp"),
}


def test_units_share_their_device_code():
    files = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".h", ".cpp"))]
    text = {f: open(os.path.join(CSRC, f)).read() for f in files}
    for what, (pattern, owner) in ONE_DEFINITION.items():
        found = {f: len(re.findall(pattern, t)) for f, t in text.items() if re.search(pattern, t)}
        assert found == {owner: 1}, (what, found)
    for fn in ("key_of", "same_key", "tile_origin", "ray_tile_pixel", "lum", "stage_tile", "add_tap", "add_prefilter_tap", "finish", "usable",
               "filter_tile", "filter_gather"):
        defined = [f for f, t in text.items() if re.search(r"TDT_DEV\s+\w+\s+" + fn + r"\(", t)]
        assert defined == ["denoise_device.hpp"], (fn, defined)
    # the four filter kernels are instantiations of the tile and the gather body; all three staged kernels go through the one staging loop
    assert "filter_tile<S, false>(" in text["tdt_denoise.hip"] and "filter_gather<false>(" in text["tdt_denoise.hip"]
    assert "filter_tile<S, true>(" in text["tdt_variance.hip"] and "filter_gather<true>(" in text["tdt_variance.hip"]
    assert "stage_tile<kVarRadius>(" in text["tdt_variance.hip"] and text["denoise_device.hpp"].count("stage_tile<2 * S>(") == 1
    # one pass loop: an entry point hands run_passes its launcher (the tile kernel or the gather) and launches nothing else itself
    for unit, entry in (("tdt_denoise.hip", "tdt_image_denoise"), ("tdt_variance.hip", "tdt_image_denoise_variance")):
        body = re.search(r"\nint " + entry + r"\(.*?\n\}\n", text[unit], re.S).group(0)
        before, handed = body.split("return tdt::run_passes(")
        assert "hipLaunchKernelGGL" not in before and handed.count("hipLaunchKernelGGL") == 2, entry
        assert not re.search(r"\bfor \(|hipGetLastError|hipMemcpy|hipSetDevice", body), entry
    assert "hipMalloc" not in text["tdt_variance.hip"]
    # both reprojection kernels live with the host code that launches them
    assert "reproject_body<false>(" in text["tdt_reproject.hip"] and "reproject_body<true>(" in text["tdt_reproject.hip"]
    assert "reproject_device.hpp" not in text["tdt_variance.hip"] and "reproject_body" not in text["tdt_variance.hip"] and not any("reproject_moments_launch" in t for t in text.values())


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
