// Luminance variance and the variance-guided filter (include/tdt_rt.h, tdt_image_variance / tdt_image_denoise_variance), and the
// kernel of tdt_image_reproject_moments, which feeds the variance its temporal moments.
//
// The variance of a pixel's luminance lives in the image's alpha channel, which neither the key-only filter nor the resolve uses,
// so a tap of the filter is still one 16-byte load.  tdt_image_variance writes it: from the temporal moments where a pixel has
// enough frames behind it, from the 7x7 same-key neighbourhood elsewhere — a block stages one luminance and the key of its 32x8
// tile and a 3-texel halo in LDS, so lum is computed once per texel.  It stores the alpha word alone and loads rgb alone: a lane
// never reads a word another lane writes.
//
// The filter is tdt_denoise.hip's a-trous frame (its tile, key, scratch sequence: denoise_device.hpp, denoise_sequence) with a
// second edge-stopping weight, max(lim - d^2, 0), lim = sigma^2 * (3x3 prefiltered variance of the centre) + floor: compactly
// supported, no exp, no per-tap divide, and its normalising 1 / lim cancels in num / den.  Steps 1 and 2 stage colour, key and
// luminance in LDS (36 B per texel, 22.5 KiB at step 2); steps >= 4 gather.  The tap order and the operation order are the
// header's, so every kernel here gives the bits of tests/variance_model.py.
#include <cmath>
#include <string>

#include "tdt_internal.hpp"
#include "denoise_device.hpp"
#include "reproject_device.hpp"

namespace tdt {

constexpr int kVarRadius = 3;                        // the spatial estimate's window is 7x7

__global__ __launch_bounds__(256) void variance_kernel(float *img, const uint4 *__restrict__ guide, const float4 *__restrict__ moments,
                                                       float min_frames, int w, int h, uint32_t tiles_x) {
  constexpr int TW = kTileW + 2 * kVarRadius, TH = kTileH + 2 * kVarRadius;
  __shared__ float s_lum[TW * TH];
  __shared__ uint4 s_key[TW * TH];
  int x0, y0;
  tile_origin(tiles_x, x0, y0);
  for (int t = (int)threadIdx.x; t < TW * TH; t += 256) {
    const int ly = t / TW, lx = t - ly * TW;
    const int gx = x0 - kVarRadius + lx, gy = y0 - kVarRadius + ly;
    float l = 0.f;
    uint4 k = make_uint4(0u, 0u, 0u, 0u);
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const size_t p = (size_t)gy * (size_t)w + (size_t)gx;
      const float *c = img + 4 * p;                  // rgb only: alpha is what this call writes
      l = lum(c[0], c[1], c[2]); k = key_of(guide[p]);
    }
    s_lum[t] = l; s_key[t] = k;
  }
  __syncthreads();
  const int lx = (int)(threadIdx.x % kTileW), ly = (int)(threadIdx.x / kTileW);
  const int x = x0 + lx, y = y0 + ly;
  if (x >= w || y >= h) return;
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const int centre = (ly + kVarRadius) * TW + lx + kVarRadius;
  const uint4 ck = s_key[centre];
  float a = 0.0f;
  if (ck.x != 0u) {
    bool temporal = false;
    if (moments) {
      const float4 m = moments[p];
      if (m.z >= min_frames) {
        const float mu = m.x / m.z, e2 = m.y / m.z;
        float v = e2 - mu * mu;
        v = v > 0.f ? v : 0.f;
        a = v / m.z;
        temporal = true;
      }
    }
    if (!temporal) {
      float K = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int j = -kVarRadius; j <= kVarRadius; j++)
#pragma unroll
        for (int i = -kVarRadius; i <= kVarRadius; i++) {
          const int t = centre + j * TW + i;
          if (same_key(s_key[t], ck)) {
            const float l = s_lum[t];
            K = K + 1.0f; s1 = s1 + l; s2 = s2 + l * l;
          }
        }
      const float mu = s1 / K;
      const float v = s2 / K - mu * mu;
      a = v > 0.f ? v : 0.f;
    }
  }
  img[4 * p + 3] = a;
}

// ---- the variance-guided filter ----
struct VarSums { float r, g, b, den, vnum; };
// one same-key tap: kept when d2 < lim (NaN fails); w = (k[j] * k[i]) * (lim - d2), every operation rounded on its own
TDT_DEV void add_var_tap(VarSums &s, int j, int i, const float4 c, float l, float lP, float lim) {
  const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  const float d = l - lP;
  const float d2 = d * d;
  if (d2 < lim) {
    const float w = (k[j] * k[i]) * (lim - d2);
    s.r = s.r + w * c.x; s.g = s.g + w * c.y; s.b = s.b + w * c.z;
    s.den = s.den + w;
    s.vnum = s.vnum + (w * w) * c.w;
  }
}
TDT_DEV float4 finish_var(const VarSums &s) { return make_float4(s.r / s.den, s.g / s.den, s.b / s.den, s.vnum / (s.den * s.den)); }
// one same-key tap of the 3x3 prefilter of the variance, g = {1/4, 1/2, 1/4}
TDT_DEV void add_prefilter_tap(float &gnum, float &gden, int j, int i, float a) {
  const float g[3] = {0.25f, 0.5f, 0.25f};
  const float wg = g[j] * g[i];
  gnum = gnum + wg * a; gden = gden + wg;
}
TDT_DEV bool usable(float lim) { return lim > 0.f && lim < INFINITY; }

// steps 1 and 2: the tile and its halo of 2 * S texels through LDS (the distance-1 taps of the prefilter lie inside it)
template <int S>
__global__ __launch_bounds__(256) void denoise_variance_tile_kernel(const float4 *__restrict__ in, const uint4 *__restrict__ guide,
                                                                    float4 *__restrict__ out, float s2, float floor, int w, int h,
                                                                    uint32_t tiles_x) {
  constexpr int TW = kTileW + 4 * S, TH = kTileH + 4 * S;
  __shared__ float4 s_col[TW * TH];
  __shared__ uint4 s_key[TW * TH];
  __shared__ float s_lum[TW * TH];
  int x0, y0;
  tile_origin(tiles_x, x0, y0);
  for (int t = (int)threadIdx.x; t < TW * TH; t += 256) {
    const int ly = t / TW, lx = t - ly * TW;
    const int gx = x0 - 2 * S + lx, gy = y0 - 2 * S + ly;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    uint4 k = make_uint4(0u, 0u, 0u, 0u);
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const size_t p = (size_t)gy * (size_t)w + (size_t)gx;
      c = in[p]; k = key_of(guide[p]);
    }
    s_col[t] = c; s_key[t] = k; s_lum[t] = lum(c.x, c.y, c.z);
  }
  __syncthreads();
  const int lx = (int)(threadIdx.x % kTileW), ly = (int)(threadIdx.x / kTileW);
  const int x = x0 + lx, y = y0 + ly;
  if (x >= w || y >= h) return;
  const int centre = (ly + 2 * S) * TW + lx + 2 * S;
  const uint4 ck = s_key[centre];
  float4 o = s_col[centre];
  if (ck.x != 0u) {
    float gnum = 0.f, gden = 0.f;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const int t = centre + (j - 1) * TW + (i - 1);
        if (same_key(s_key[t], ck)) add_prefilter_tap(gnum, gden, j, i, s_col[t].w);
      }
    const float lim = s2 * (gnum / gden) + floor;
    if (usable(lim)) {
      const float lP = s_lum[centre];
      VarSums s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 5; j++)
#pragma unroll
        for (int i = 0; i < 5; i++) {
          const int t = centre + (j - 2) * S * TW + (i - 2) * S;
          if (same_key(s_key[t], ck)) add_var_tap(s, j, i, s_col[t], s_lum[t], lP, lim);
        }
      o = finish_var(s);
    }
  }
  out[(size_t)y * (size_t)w + (size_t)x] = o;
}

// steps >= 4: every lane gathers its nine distance-1 taps and its 25 taps
__global__ __launch_bounds__(256) void denoise_variance_gather_kernel(const float4 *__restrict__ in, const uint4 *__restrict__ guide,
                                                                      float4 *__restrict__ out, float s2, float floor, int w, int h, int step,
                                                                      uint32_t tiles_x) {
  int x0, y0;
  tile_origin(tiles_x, x0, y0);
  const int x = x0 + (int)(threadIdx.x % kTileW), y = y0 + (int)(threadIdx.x / kTileW);
  if (x >= w || y >= h) return;
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const uint4 ck = key_of(guide[p]);
  const float4 cc = in[p];
  float4 o = cc;
  if (ck.x != 0u) {
    float gnum = 0.f, gden = 0.f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int qy = y + j - 1;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const int qx = x + i - 1;
        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
        const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
        if (same_key(key_of(guide[q]), ck)) add_prefilter_tap(gnum, gden, j, i, in[q].w);
      }
    }
    const float lim = s2 * (gnum / gden) + floor;
    if (usable(lim)) {
      const float lP = lum(cc.x, cc.y, cc.z);
      VarSums s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 5; j++) {
        const long long qy = (long long)y + (long long)(j - 2) * step;
#pragma unroll
        for (int i = 0; i < 5; i++) {
          const long long qx = (long long)x + (long long)(i - 2) * step;
          if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
          const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
          if (same_key(key_of(guide[q]), ck)) {
            const float4 c = in[q];
            add_var_tap(s, j, i, c, lum(c.x, c.y, c.z), lP, lim);
          }
        }
      }
      o = finish_var(s);
    }
  }
  out[p] = o;
}

// ---- the moments form of temporal reprojection (the call itself is tdt_reproject.hip's) ----
__global__ __launch_bounds__(256) void reproject_moments_kernel(const TraceParams P, int sample, const ReprojectArgs A,
                                                                const uint4 *__restrict__ guide, const float4 *sums,
                                                                const uint4 *__restrict__ prev_guide, const float4 *__restrict__ prev_hist,
                                                                float4 *__restrict__ hist_out, float4 *mean_out, int w, int h, uint32_t tiles_x,
                                                                unsigned long long *__restrict__ counts,
                                                                const float4 *__restrict__ prev_moments, float4 *__restrict__ moments_out, float mf) {
  reproject_body<true>(P, sample, A, guide, sums, prev_guide, prev_hist, hist_out, mean_out, w, h, tiles_x, counts, prev_moments, moments_out, mf);
}

void reproject_moments_launch(dim3 grid, hipStream_t stream, const TraceParams &P, int sample, const ReprojectArgs &A, const uint4 *guide,
                              const float4 *sums, const uint4 *prev_guide, const float4 *prev_hist, float4 *hist_out, float4 *mean_out, int w, int h,
                              uint32_t tiles_x, unsigned long long *counts, const float4 *prev_moments, float4 *moments_out, float mf) {
  hipLaunchKernelGGL(reproject_moments_kernel, grid, dim3(256), 0, stream, P, sample, A, guide, sums, prev_guide, prev_hist, hist_out, mean_out, w, h,
                     tiles_x, counts, prev_moments, moments_out, mf);
}

}  // namespace tdt

extern "C" {

int tdt_image_variance(tdt_image *img, const tdt_image *guide, const tdt_image *moments, float min_frames, uint32_t flags) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  if (!guide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide image");
  if (guide->ctx != ctx || (moments && moments->ctx != ctx)) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "an image belongs to another context");
  const tdt_image *a = tdt::device_image(img), *g = tdt::device_image(guide), *mo = moments ? tdt::device_image(moments) : nullptr;
  if (a->w != g->w || a->h != g->h || (mo && (mo->w != a->w || mo->h != a->h)))
    return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "image, guide and moments differ in size");
  if (img == guide || tdt::overlap(a, g) || (mo && (moments == img || moments == guide || tdt::overlap(mo, a) || tdt::overlap(mo, g))))
    return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "two of the images are one (or share memory)");
  if (!(min_frames >= 1.0f)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "min_frames must be at least 1");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  const unsigned long long tiles_x = ((unsigned long long)a->w + tdt::kTileW - 1) / tdt::kTileW,
                           tiles_y = ((unsigned long long)a->h + tdt::kTileH - 1) / tdt::kTileH;
  if (tiles_x * tiles_y > 0x7FFFFFFFull) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "image too large");
  if (tiles_x * tiles_y == 0) return TDT_OK;
  tdt_ctx *m = tdt::first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  hipLaunchKernelGGL(tdt::variance_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, m->stream, a->dev, (const uint4 *)g->dev,
                     mo ? (const float4 *)mo->dev : nullptr, min_frames, a->w, a->h, (uint32_t)tiles_x);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_image_denoise_variance(tdt_image *img, const tdt_image *guide, int passes, float sigma, float floor, uint32_t flags) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  if (!guide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide image");
  if (guide->ctx != ctx) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "guide image belongs to another context");
  const tdt_image *a = tdt::device_image(img), *g = tdt::device_image(guide);
  if (a->w != g->w || a->h != g->h) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "image and guide differ in size");
  if (img == guide || tdt::overlap(a, g)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the guide is the image itself (or shares its memory)");
  if (passes < 0 || passes > tdt::kMaxPasses) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "passes must be 0..8");
  if (!(sigma > 0.0f) || !std::isfinite(sigma)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "sigma must be positive and finite");
  if (!(floor >= 0.0f) || !std::isfinite(floor)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "floor must be non-negative and finite");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (passes == 0) return TDT_OK;
  const unsigned long long tiles_x = ((unsigned long long)a->w + tdt::kTileW - 1) / tdt::kTileW,
                           tiles_y = ((unsigned long long)a->h + tdt::kTileH - 1) / tdt::kTileH;
  if (tiles_x * tiles_y > 0x7FFFFFFFull) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "image too large");
  if (tiles_x * tiles_y == 0) return TDT_OK;
  tdt_ctx *m = tdt::first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  float *seq[tdt::kMaxPasses + 1];
  if (int rc = tdt::denoise_sequence(ctx, m, a->dev, a->w, a->h, passes, seq)) return rc;
  const float s2 = sigma * sigma;
  const uint4 *G = (const uint4 *)g->dev;
  const dim3 grid((unsigned)(tiles_x * tiles_y)), block(256);
  for (int p = 0; p < passes; p++) {
    const float4 *src = (const float4 *)seq[p];
    float4 *dst = (float4 *)seq[p + 1];
    if (p == 0) hipLaunchKernelGGL(tdt::denoise_variance_tile_kernel<1>, grid, block, 0, m->stream, src, G, dst, s2, floor, a->w, a->h, (uint32_t)tiles_x);
    else if (p == 1) hipLaunchKernelGGL(tdt::denoise_variance_tile_kernel<2>, grid, block, 0, m->stream, src, G, dst, s2, floor, a->w, a->h, (uint32_t)tiles_x);
    else hipLaunchKernelGGL(tdt::denoise_variance_gather_kernel, grid, block, 0, m->stream, src, G, dst, s2, floor, a->w, a->h, 1 << p, (uint32_t)tiles_x);
  }
  TDT_HIP(ctx, hipGetLastError());
  if (seq[passes] != seq[0])
    TDT_HIP(ctx, hipMemcpyAsync(seq[0], seq[passes], (size_t)a->w * (size_t)a->h * 16, hipMemcpyDeviceToDevice, m->stream));
  return TDT_OK;
}

}  // extern "C"
