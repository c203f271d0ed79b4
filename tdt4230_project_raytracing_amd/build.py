"""Build recipes for the in-tree shared libraries (explicit compiler invocations, outputs
stay in-tree so they travel to the GPU box with the snapshot)."""
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")

HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# -ffp-contract=off and IEEE divide/sqrt are PARITY flags, not tuning knobs: the reference's
# arithmetic is unfused and correctly rounded (DESIGN.md §4 "Parity flags").
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wall", "-Wextra",
             # measured: SLP-packed v_pk_*_f32 costs 6 % here (register-pair shuffles around scalar vec3 code)
             "-fno-slp-vectorize"]
HOST_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off"]


def _newer(out, srcs):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in srcs)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    return r.stdout + r.stderr


def build_host(force=False):
    out = os.path.join(_HERE, "libtdthost.so")
    srcs = [os.path.join(CSRC, "host_scene.cpp"), os.path.join(CSRC, "host_view.cpp"), os.path.join(CSRC, "host_mesh.cpp"),
            os.path.join(CSRC, "host_xform.cpp"), os.path.join(INCLUDE, "tdt_host.h"), os.path.join(INCLUDE, "tdt_rt.h"), os.path.abspath(__file__)]
    if force or _newer(out, srcs):
        _run(["g++"] + HOST_FLAGS + ["-I", INCLUDE] + srcs[:4] + ["-o", out, "-lz"])      # zlib: the PNG writer (§8f-4)
    return out


DEVICE_UNITS = ("tdt_rt.hip", "tdt_multi.hip", "tdt_build.hip", "tdt_edit.hip", "tdt_query.hip", "tdt_compact.hip",
                "tdt_region.hip", "tdt_connect.hip", "tdt_morph.hip", "tdt_mesh.hip", "tdt_fill.hip", "tdt_surface.hip",
                "tdt_distance.hip", "tdt_bitvol.hip", "tdt_xform.hip", "tdt_geodesic.hip", "tdt_voxlist.hip", "tdt_denoise.hip",
                "tdt_reproject.hip", "tdt_variance.hip", "tdt_upsample.hip", "tdt_adaptive.hip", "tdt_select.hip",
                "tdt_screen.hip", "tdt_smooth.hip", "tdt_stroke.hip", "tdt_faces.hip")
DEVICE_HEADERS = ("trace_device.hpp", "trace_params.h", "tdt_internal.hpp", "device_scan.hpp", "region_device.hpp", "bitvol_device.hpp",
                  "query_device.hpp", "denoise_device.hpp", "reproject_device.hpp", "surface_device.hpp", "unionfind_device.hpp")


def build_device(force=False, extra_flags=(), out=None):
    """libtdtrt.so: one object per translation unit (compiled side by side: the trace kernels take ~15 s, the rest
    seconds), then one link.  Objects live in csrc/obj/ (git- and gpurun-ignored); only the .so travels."""
    out = out or os.path.join(_HERE, "libtdtrt.so")
    hdrs = [os.path.join(CSRC, f) for f in DEVICE_HEADERS] + [os.path.join(INCLUDE, "tdt_rt.h"), os.path.abspath(__file__)]
    srcs = [os.path.join(CSRC, f) for f in DEVICE_UNITS]
    if not (force or extra_flags or _newer(out, srcs + hdrs)):
        return out
    objdir = os.path.join(CSRC, "obj" + ("_" + str(abs(hash(tuple(extra_flags))) % 100000) if extra_flags else ""))
    os.makedirs(objdir, exist_ok=True)
    compile_flags = [f for f in HIP_FLAGS if f != "-shared"] + list(extra_flags)
    jobs = []
    for src in srcs:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        if force or extra_flags or _newer(obj, [src] + hdrs):
            jobs.append((subprocess.Popen([HIPCC] + compile_flags + ["-I", INCLUDE, "-I", CSRC, "-c", src, "-o", obj],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), src))
    for p, src in jobs:
        log, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("build failed: " + src + "\n" + log)
    objs = [os.path.join(objdir, os.path.basename(src) + ".o") for src in srcs]
    _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out, "-ldl"])
    return out


STATS_LIB = os.path.join(_HERE, "libtdtrt_stats.so")


def build_stats(force=False):
    """libtdtrt_stats.so: the same library compiled with -DTDT_STATS, whose product trace kernels count their passes (tdt_debug_stats;
    tools/loss_budget.py, tests/test_gpu_five_waves.py load it through TDT_LIB in a process of their own).  Never the product library."""
    hdrs = [os.path.join(CSRC, f) for f in DEVICE_HEADERS] + [os.path.join(INCLUDE, "tdt_rt.h"), os.path.abspath(__file__)]
    srcs = [os.path.join(CSRC, f) for f in DEVICE_UNITS]
    if force or _newer(STATS_LIB, srcs + hdrs):
        build_device(extra_flags=("-DTDT_STATS",), out=STATS_LIB)
    return STATS_LIB


def build_demo(force=False):
    """tdt_demo: the reference's main.rs, headless, written against include/renderer.hpp (C++ host mirror)."""
    out = os.path.join(_HERE, "tdt_demo")
    srcs = [os.path.join(CSRC, "demo_main.cpp"), os.path.join(INCLUDE, "renderer.hpp"), os.path.join(INCLUDE, "tdt_rt.h"),
            os.path.join(INCLUDE, "tdt_host.h"), os.path.abspath(__file__)]
    if force or _newer(out, srcs):
        rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib")
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", INCLUDE, srcs[0], "-o", out, "-L", _HERE, "-ltdtrt", "-ltdthost",
              "-Wl,-rpath,$ORIGIN", "-Wl,-rpath-link," + rocm_lib])
    return out


def build_selftest(force=False):
    """libtdtprims_selftest.so: the test-only harness over the device scan and the radix sort (csrc/prims_selftest.hip).
    The scan is compiled into it from device_scan.hpp with the product's flags; the sort is libtdtrt.so's own, found next
    to it at load time.  Not part of libtdtrt.so or its ABI."""
    out = os.path.join(_HERE, "libtdtprims_selftest.so")
    src = os.path.join(CSRC, "prims_selftest.hip")
    deps = [src, os.path.join(CSRC, "device_scan.hpp"), os.path.join(CSRC, "tdt_internal.hpp"),
            os.path.join(INCLUDE, "tdt_rt.h"), os.path.abspath(__file__)]
    if force or _newer(out, deps):
        _run([HIPCC] + HIP_FLAGS + ["-I", INCLUDE, "-I", CSRC, src, "-o", out, "-L", _HERE, "-ltdtrt", "-Wl,-rpath,$ORIGIN"])
    return out


def build_all(force=False):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(2) as pool:               # (the two device libraries side by side: each is bound by the trace unit's compile)
        stats = pool.submit(build_stats, force)
        host_lib, device_lib = build_host(force), build_device(force)
        stats_lib = stats.result()
    return host_lib, device_lib, build_demo(force), build_selftest(force), stats_lib
