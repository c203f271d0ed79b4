// Temporal reprojection (include/tdt_rt.h, tdt_compute_view / tdt_image_reproject / tdt_image_reproject_moments /
// tdt_debug_reproject_counts).
//
// One lane per pixel of the current frame: the world point its guide texel stands for (primary ray origin + t * direction) is
// projected into an earlier frame's view, and that frame's history texel is added to this frame's sums when its guide texel carries
// the same key.  Voxel faces are axis-aligned planes, so an equal key (kind, material, plane) means "the old pixel saw this face
// at this point" with no tolerance.  The projection is three dot products with the rows of the inverse of (horizontal, vertical,
// lower_left_corner - origin) scaled by its determinant (the host computes them once per call, in double), and two divides.
// The arithmetic and its order are the header's, so a numpy model gives the same bits.  Both kernels, reproject_kernel and the
// moments form that feeds tdt_image_variance its temporal moments, instantiate the one body of reproject_device.hpp; the host
// frame around them (handles, grid, camera program) is tdt_internal.hpp's, shared with tdt_denoise.hip and tdt_variance.hip.
//
// The kernel is a gather bound by memory: 32 B read and 16 or 32 B written per pixel at home, and up to 32 B gathered from the old
// frame.  A block covers the guide kernel's 16x16 tile (denoise_device.hpp), so that the old frame's texels its lanes ask for lie
// close together too.
#include <cmath>
#include <string>

#include "tdt_internal.hpp"
#include "trace_params.h"
#include "trace_device.hpp"
#include "reproject_device.hpp"

namespace tdt {

constexpr int kMaxPrevSide = 1 << 24;                // (float)side is exact up to here: fx < (float)prev_w then bounds (int)fx

__global__ __launch_bounds__(256) void reproject_kernel(const TraceParams P, int sample, const ReprojectArgs A, const uint4 *__restrict__ guide,
                                                        const float4 *sums, const uint4 *__restrict__ prev_guide,
                                                        const float4 *__restrict__ prev_hist, float4 *__restrict__ hist_out, float4 *mean_out,
                                                        int w, int h, uint32_t tiles_x, unsigned long long *__restrict__ counts) {
  reproject_body<false>(P, sample, A, guide, sums, prev_guide, prev_hist, hist_out, mean_out, w, h, tiles_x, counts, nullptr, nullptr, 0.f);
}

// the moments form (tdt_image_reproject_moments): the arguments above, then the earlier frame's moments or null, the moments image
// to write, and mf = max_samples / (float)spp
__global__ __launch_bounds__(256) void reproject_moments_kernel(const TraceParams P, int sample, const ReprojectArgs A,
                                                                const uint4 *__restrict__ guide, const float4 *sums,
                                                                const uint4 *__restrict__ prev_guide, const float4 *__restrict__ prev_hist,
                                                                float4 *__restrict__ hist_out, float4 *mean_out, int w, int h, uint32_t tiles_x,
                                                                unsigned long long *__restrict__ counts,
                                                                const float4 *__restrict__ prev_moments, float4 *__restrict__ moments_out, float mf) {
  reproject_body<true>(P, sample, A, guide, sums, prev_guide, prev_hist, hist_out, mean_out, w, h, tiles_x, counts, prev_moments, moments_out, mf);
}

// Ru, Rv, Rw of the header from a view's fp32 fields, in double, one rounding per operation (the build does not contract), then
// rounded to fp32, with the origin and (float)(image_width - 1), (float)(image_height - 1); false: the determinant is zero or not finite
bool view_rows(const tdt_view &v, ViewRows &A) {
  double a[3], b[3], c[3];
  for (int i = 0; i < 3; i++) {
    a[i] = (double)v.horizontal[i]; b[i] = (double)v.vertical[i];
    c[i] = (double)v.lower_left_corner[i] - (double)v.origin[i];
  }
  const auto cross = [](const double *u, const double *w, double *out) {
    for (int i = 0; i < 3; i++) {
      const int j = (i + 1) % 3, k = (i + 2) % 3;
      const double p = u[j] * w[k], q = u[k] * w[j];
      out[i] = p - q;
    }
  };
  double ru[3], rv[3], rw[3];
  cross(b, c, ru); cross(c, a, rv); cross(a, b, rw);
  const double pz = c[2] * rw[2], py = c[1] * rw[1], px = c[0] * rw[0];
  const double det = (pz + py) + px;
  if (!std::isfinite(det) || det == 0.0) return false;
  const double sign = det < 0.0 ? -1.0 : 1.0;
  for (int i = 0; i < 3; i++) {
    A.ru[i] = (float)(sign * ru[i]); A.rv[i] = (float)(sign * rv[i]); A.rw[i] = (float)(sign * rw[i]);
    A.org[i] = v.origin[i];
  }
  A.sx = (float)(v.image_width - 1); A.sy = (float)(v.image_height - 1);
  return true;
}

void reproject_counts_destroy(tdt_ctx *ctx) {
  if (ctx->reproject_counts) (void)hipFree(ctx->reproject_counts);
  ctx->reproject_counts = nullptr;
}

}  // namespace tdt

extern "C" {

int tdt_compute_view(const tdt_compute *c, tdt_view *out) {
  if (!c) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = c->ctx;
  if (!out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null view");
  if (c->kind != TDT_PROGRAM_RAYTRACER) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "a view needs a raytracer program (its camera)");
  TraceParams P;
  tdt::query_camera(tdt::camera_program(c), P);                          // the one place that reads a program's camera
  for (int i = 0; i < 3; i++) {
    out->origin[i] = P.org[i]; out->lower_left_corner[i] = P.llc[i]; out->horizontal[i] = P.hor[i]; out->vertical[i] = P.ver[i];
  }
  out->image_width = P.image_width; out->image_height = P.image_height;
  return TDT_OK;
}

// both reprojection calls; with_moments: prev_moments comes and goes with the other prev_*, moments_out is required
static int reproject_run(tdt_compute *c, int sample, const tdt_image *guide, const tdt_image *sums, int spp, const tdt_view *prev_view,
                         const tdt_image *prev_guide, const tdt_image *prev_hist, const tdt_image *prev_moments, float max_samples,
                         tdt_image *hist_out, tdt_image *moments_out, tdt_image *mean_out, uint32_t flags, bool with_moments) {
  if (!c) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = c->ctx;
  if (!guide || !sums || !hist_out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide, sums or history image");
  if (with_moments && !moments_out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null moments image");
  const bool has_prev = prev_view || prev_guide || prev_hist || prev_moments;
  if (has_prev && !(prev_view && prev_guide && prev_hist && (prev_moments || !with_moments)))
    return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, with_moments ? "the earlier frame's view, guide, history and moments come together or not at all"
                                                              : "the earlier frame's view, guide and history come together or not at all");
  if (c->kind != TDT_PROGRAM_RAYTRACER) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "reprojection needs a raytracer program (its camera)");
  constexpr int N = 8, SIZED = 5;                                        // (the first five share the guide's size; mean_out may be sums)
  const tdt_image *handles[N] = {guide, sums, hist_out, mean_out, moments_out, prev_guide, prev_hist, prev_moments}, *im[N];
  if (int rc = tdt::images_of_context(ctx, handles, N, "an image belongs to another context")) return rc;
  if (c->part_rank != 0 || c->part_world != 1)
    return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "reprojection works on images, not tile buffers: the program's partition must be (0, 1)");
  if (sample < 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "negative sample index");
  if (spp < 1) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "spp must be at least 1");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (!(max_samples >= 1.0f)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "max_samples must be at least 1");
  if (int rc = tdt::images_fit(ctx, handles, N, SIZED, im, with_moments ? "guide, sums, history, moments and mean differ in size"
                                                                        : "guide, sums, history and mean differ in size",
                               "two of the images are one (or share memory)", 1, 3))
    return rc;
  const tdt_image *g = im[0], *s = im[1], *ho = im[2], *mo = im[3], *mm = im[4], *pg = im[5], *ph = im[6], *pm = im[7];
  tdt::ReprojectArgs A = {};
  if (has_prev) {
    if (pg->w != ph->w || pg->h != ph->h) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier guide and history differ in size");
    if (pm && (pm->w != pg->w || pm->h != pg->h)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier guide and moments differ in size");
    if (pg->w > tdt::kMaxPrevSide || pg->h > tdt::kMaxPrevSide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier images are too large");
    if (prev_view->image_width < 2 || prev_view->image_height < 2)
      return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier view's image_width and image_height must be at least 2");
    if (!tdt::view_rows(*prev_view, A.view)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier view is degenerate (determinant zero or not finite)");
    A.fpw = (float)pg->w; A.fph = (float)pg->h; A.pw = pg->w;
    A.has_prev = 1;
  }
  A.fspp = (float)spp; A.max_samples = max_samples;
  dim3 grid;
  uint32_t tiles_x;
  if (int rc = tdt::image_grid(ctx, g->w, g->h, tdt::kRayTile, tdt::kRayTile, "image too large", grid, tiles_x)) return rc;
  const tdt_compute *cam = tdt::camera_program(c);
  tdt_ctx *m = cam->ctx;
  TraceParams P = {};
  tdt::query_camera(cam, P);
  TDT_HIP(ctx, hipSetDevice(m->device));
  if (!m->reproject_counts) {
    const hipError_t e = hipMalloc((void **)&m->reproject_counts, 4 * sizeof(unsigned long long));
    if (e != hipSuccess) { m->reproject_counts = nullptr; return tdt::hip_fail(ctx, e, "hipMalloc (reprojection counts)"); }
  }
  TDT_HIP(ctx, hipMemsetAsync(m->reproject_counts, 0, 4 * sizeof(unsigned long long), m->stream));
  const uint4 *G = (const uint4 *)g->dev, *PG = has_prev ? (const uint4 *)pg->dev : nullptr;
  const float4 *S = (const float4 *)s->dev, *PH = has_prev ? (const float4 *)ph->dev : nullptr;
  float4 *HO = (float4 *)ho->dev, *MO = mo ? (float4 *)mo->dev : nullptr;
  if (with_moments)
    hipLaunchKernelGGL(tdt::reproject_moments_kernel, grid, dim3(256), 0, m->stream, P, sample, A, G, S, PG, PH, HO, MO, g->w, g->h, tiles_x,
                       m->reproject_counts, has_prev ? (const float4 *)pm->dev : nullptr, (float4 *)mm->dev, max_samples / (float)spp);
  else
    hipLaunchKernelGGL(tdt::reproject_kernel, grid, dim3(256), 0, m->stream, P, sample, A, G, S, PG, PH, HO, MO, g->w, g->h, tiles_x,
                       m->reproject_counts);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_image_reproject(tdt_compute *c, int sample, const tdt_image *guide, const tdt_image *sums, int spp, const tdt_view *prev_view,
                        const tdt_image *prev_guide, const tdt_image *prev_hist, float max_samples, tdt_image *hist_out, tdt_image *mean_out,
                        uint32_t flags) {
  return reproject_run(c, sample, guide, sums, spp, prev_view, prev_guide, prev_hist, nullptr, max_samples, hist_out, nullptr, mean_out, flags, false);
}

int tdt_image_reproject_moments(tdt_compute *c, int sample, const tdt_image *guide, const tdt_image *sums, int spp, const tdt_view *prev_view,
                                const tdt_image *prev_guide, const tdt_image *prev_hist, const tdt_image *prev_moments, float max_samples,
                                tdt_image *hist_out, tdt_image *moments_out, tdt_image *mean_out, uint32_t flags) {
  return reproject_run(c, sample, guide, sums, spp, prev_view, prev_guide, prev_hist, prev_moments, max_samples, hist_out, moments_out, mean_out,
                       flags, true);
}

int tdt_image_clear(tdt_image *img) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  // a multi-device context keeps a bound image's running sums in its members' tile buffers, which this handle does not reach
  if (ctx->multi) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "tdt_image_clear works on a single-device context");
  TDT_HIP(ctx, hipSetDevice(ctx->device));
  TDT_HIP(ctx, hipMemsetAsync(img->dev, 0, (size_t)img->w * (size_t)img->h * 16, ctx->stream));
  return TDT_OK;
}

int tdt_debug_reproject_counts(tdt_ctx *ctx, uint64_t out[4]) {
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null counts");
  tdt_ctx *m = tdt::first_member(ctx);
  unsigned long long host[4] = {0, 0, 0, 0};
  TDT_HIP(ctx, hipSetDevice(m->device));
  if (m->reproject_counts) TDT_HIP(ctx, hipMemcpyAsync(host, m->reproject_counts, sizeof host, hipMemcpyDeviceToHost, m->stream));
  TDT_HIP(ctx, hipStreamSynchronize(m->stream));
  for (int i = 0; i < 4; i++) out[i] = host[i];
  return TDT_OK;
}

}  // extern "C"
