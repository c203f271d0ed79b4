// Temporal reprojection (include/tdt_rt.h, tdt_compute_view / tdt_image_reproject / tdt_debug_reproject_counts).
//
// One lane per pixel of the current frame: the world point its guide texel stands for (primary ray origin + t * direction) is
// projected into an earlier frame's view, and that frame's history texel is added to this frame's sums when its guide texel carries
// the same key.  Voxel faces are axis-aligned planes, so an equal key (kind, material, plane) means "the old pixel saw this face
// at this point" with no tolerance.  The projection is three dot products with the rows of the inverse of (horizontal, vertical,
// lower_left_corner - origin) scaled by its determinant (the host computes them once per call, in double), and two divides.
// The arithmetic and its order are the header's, so a numpy model gives the same bits.
//
// The kernel is a gather bound by memory: 32 B read and 16 or 32 B written per pixel at home, and up to 32 B gathered from the old
// frame.  A block covers a 16x16 tile, so that the old frame's texels its lanes ask for lie close together too.
#include <cmath>
#include <string>

#include "tdt_internal.hpp"
#include "trace_params.h"
#include "trace_device.hpp"

namespace tdt {

constexpr uint32_t kReprojectTile = 16;              // as the guide kernel's tile
constexpr int kMaxPrevSide = 1 << 24;                // (float)side is exact up to here: fx < (float)prev_w then bounds (int)fx

struct ReprojectArgs {
  float ru[3], rv[3], rw[3];                         // rows of det * inverse(a | b | c) of the earlier view, det > 0
  float org[3];                                      // its origin
  float sx, sy;                                      // (float)(image_width - 1), (float)(image_height - 1) of the earlier view
  float fpw, fph;                                    // (float) sizes of the earlier images
  int pw;                                            // their row length
  int has_prev;
  float fspp, max_samples;
};

__global__ __launch_bounds__(256) void reproject_kernel(const TraceParams P, int sample, const ReprojectArgs A, const uint4 *__restrict__ guide,
                                                        const float4 *sums, const uint4 *__restrict__ prev_guide,
                                                        const float4 *__restrict__ prev_hist, float4 *__restrict__ hist_out, float4 *mean_out,
                                                        int w, int h, uint32_t tiles_x, unsigned long long *__restrict__ counts) {
  __shared__ uint32_t s_count[4];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = (int)(tx * kReprojectTile + (threadIdx.x & (kReprojectTile - 1))), y = (int)(ty * kReprojectTile + threadIdx.x / kReprojectTile);
  // what became of this lane's pixel: 0 = outside the image or not keyed, 1 = found, 2 = rejected by key or hn, 3 = by nw or off-screen
  uint32_t fate = 0u;
  bool keyed = false;
  if (x < w && y < h) {
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    const uint4 g = guide[p];
    const float4 s = sums[p];
    float4 o = make_float4(s.x, s.y, s.z, A.fspp);
    keyed = g.x != 0u;
    if (keyed && A.has_prev) {
      const Ray r = primary_ray(P, x, y, sample);
      const float t = __uint_as_float(g.w);
      const float dx = (r.ox + t * r.dx) - A.org[0], dy = (r.oy + t * r.dy) - A.org[1], dz = (r.oz + t * r.dz) - A.org[2];
      const float nu = (A.ru[2] * dz + A.ru[1] * dy) + A.ru[0] * dx;
      const float nv = (A.rv[2] * dz + A.rv[1] * dy) + A.rv[0] * dx;
      const float nw = (A.rw[2] * dz + A.rw[1] * dy) + A.rw[0] * dx;
      const float fx = (nu / nw) * A.sx, fy = (nv / nw) * A.sy;
      fate = 3u;
      if (nw > 0.f && fx >= 0.f && fx < A.fpw && fy >= 0.f && fy < A.fph) {
        const size_t q = (size_t)(int)fy * (size_t)A.pw + (size_t)(int)fx;
        const uint4 k = prev_guide[q];
        fate = 2u;
        if (k.x == g.x && k.y == g.y && k.z == g.z) {
          float4 hq = prev_hist[q];
          if (hq.w > 0.f) {
            fate = 1u;
            if (hq.w > A.max_samples) {
              const float sc = A.max_samples / hq.w;
              hq.x = hq.x * sc; hq.y = hq.y * sc; hq.z = hq.z * sc; hq.w = A.max_samples;
            }
            o = make_float4(s.x + hq.x, s.y + hq.y, s.z + hq.z, A.fspp + hq.w);
          }
        }
      }
    }
    hist_out[p] = o;
    if (mean_out) mean_out[p] = make_float4(o.x / o.w, o.y / o.w, o.z / o.w, 1.0f);
  }
  // the block's counts: one LDS add per wave and counter, then one global add per counter
  const unsigned long long m0 = __ballot(keyed), m1 = __ballot(fate == 1u), m2 = __ballot(fate == 2u), m3 = __ballot(fate == 3u);
  if ((threadIdx.x & 63u) == 0u) {
    if (m0) atomicAdd(&s_count[0], (uint32_t)__popcll(m0));
    if (m1) atomicAdd(&s_count[1], (uint32_t)__popcll(m1));
    if (m2) atomicAdd(&s_count[2], (uint32_t)__popcll(m2));
    if (m3) atomicAdd(&s_count[3], (uint32_t)__popcll(m3));
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

namespace {

// Ru, Rv, Rw of the header from a view's fp32 fields, in double, one rounding per operation (the build does not contract), then
// rounded to fp32; false: the determinant is zero or not finite
bool view_rows(const tdt_view &v, ReprojectArgs &A) {
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
  return true;
}

bool overlap(const tdt_image *a, const tdt_image *b) {
  const float *ea = a->dev + (size_t)a->w * (size_t)a->h * 4, *eb = b->dev + (size_t)b->w * (size_t)b->h * 4;
  return a->dev < eb && b->dev < ea;
}

}  // namespace

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
  const tdt_compute *cam = c->replicas.empty() ? c : c->replicas[0];     // (a multi-device program: its first member's camera)
  TraceParams P;
  tdt::query_camera(cam, P);                                             // the one place that reads a program's camera
  for (int i = 0; i < 3; i++) {
    out->origin[i] = P.org[i]; out->lower_left_corner[i] = P.llc[i]; out->horizontal[i] = P.hor[i]; out->vertical[i] = P.ver[i];
  }
  out->image_width = P.image_width; out->image_height = P.image_height;
  return TDT_OK;
}

int tdt_image_reproject(tdt_compute *c, int sample, const tdt_image *guide, const tdt_image *sums, int spp, const tdt_view *prev_view,
                        const tdt_image *prev_guide, const tdt_image *prev_hist, float max_samples, tdt_image *hist_out, tdt_image *mean_out,
                        uint32_t flags) {
  if (!c) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = c->ctx;
  if (!guide || !sums || !hist_out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide, sums or history image");
  const bool has_prev = prev_view || prev_guide || prev_hist;
  if (has_prev && !(prev_view && prev_guide && prev_hist))
    return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier frame's view, guide and history come together or not at all");
  if (c->kind != TDT_PROGRAM_RAYTRACER) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "reprojection needs a raytracer program (its camera)");
  const tdt_image *handles[6] = {guide, sums, hist_out, mean_out, prev_guide, prev_hist};
  for (const tdt_image *i : handles)
    if (i && i->ctx != ctx) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "an image belongs to another context");
  if (c->part_rank != 0 || c->part_world != 1)
    return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "reprojection works on images, not tile buffers: the program's partition must be (0, 1)");
  if (sample < 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "negative sample index");
  if (spp < 1) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "spp must be at least 1");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (!(max_samples >= 1.0f)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "max_samples must be at least 1");
  const tdt_image *im[6];
  for (int i = 0; i < 6; i++) im[i] = handles[i] ? tdt::device_image(handles[i]) : nullptr;
  const tdt_image *g = im[0], *s = im[1], *ho = im[2], *mo = im[3], *pg = im[4], *ph = im[5];
  if (s->w != g->w || s->h != g->h || ho->w != g->w || ho->h != g->h || (mo && (mo->w != g->w || mo->h != g->h)))
    return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "guide, sums, history and mean differ in size");
  for (int i = 0; i < 6; i++)
    for (int j = i + 1; j < 6; j++) {
      if (!im[i] || !im[j]) continue;
      if (i == 1 && j == 3 && im[i]->dev == im[j]->dev) continue;        // mean_out == sums: in place
      if (im[i] == im[j] || tdt::overlap(im[i], im[j])) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "two of the images are one (or share memory)");
    }
  tdt::ReprojectArgs A = {};
  if (has_prev) {
    if (pg->w != ph->w || pg->h != ph->h) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier guide and history differ in size");
    if (pg->w > tdt::kMaxPrevSide || pg->h > tdt::kMaxPrevSide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier images are too large");
    if (prev_view->image_width < 2 || prev_view->image_height < 2)
      return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier view's image_width and image_height must be at least 2");
    if (!tdt::view_rows(*prev_view, A)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the earlier view is degenerate (determinant zero or not finite)");
    A.sx = (float)(prev_view->image_width - 1); A.sy = (float)(prev_view->image_height - 1);
    A.fpw = (float)pg->w; A.fph = (float)pg->h; A.pw = pg->w;
    A.has_prev = 1;
  }
  A.fspp = (float)spp; A.max_samples = max_samples;
  const unsigned long long tiles_x = ((unsigned long long)g->w + tdt::kReprojectTile - 1) / tdt::kReprojectTile,
                           tiles_y = ((unsigned long long)g->h + tdt::kReprojectTile - 1) / tdt::kReprojectTile;
  if (tiles_x * tiles_y > 0x7FFFFFFFull) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "image too large");
  const tdt_compute *cam = c->replicas.empty() ? c : c->replicas[0];     // (a multi-device program: its first member's camera)
  tdt_ctx *m = cam->ctx;
  TraceParams P = {};
  tdt::query_camera(cam, P);
  TDT_HIP(ctx, hipSetDevice(m->device));
  if (!m->reproject_counts) {
    const hipError_t e = hipMalloc((void **)&m->reproject_counts, 4 * sizeof(unsigned long long));
    if (e != hipSuccess) { m->reproject_counts = nullptr; return tdt::hip_fail(ctx, e, "hipMalloc (reprojection counts)"); }
  }
  TDT_HIP(ctx, hipMemsetAsync(m->reproject_counts, 0, 4 * sizeof(unsigned long long), m->stream));
  if (tiles_x * tiles_y == 0) return TDT_OK;                             // (an empty image: the counts of this call are zero)
  hipLaunchKernelGGL(tdt::reproject_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, m->stream, P, sample, A, (const uint4 *)g->dev,
                     (const float4 *)s->dev, has_prev ? (const uint4 *)pg->dev : nullptr, has_prev ? (const float4 *)ph->dev : nullptr,
                     (float4 *)ho->dev, mo ? (float4 *)mo->dev : nullptr, g->w, g->h, (uint32_t)tiles_x, m->reproject_counts);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
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
