// Luminance variance and the variance-guided filter (include/tdt_rt.h, tdt_image_variance / tdt_image_denoise_variance).
//
// The variance of a pixel's luminance lives in the image's alpha channel, which neither the key-only filter nor the resolve uses,
// so a tap of the filter is still one 16-byte load.  tdt_image_variance writes it: from the temporal moments where a pixel has
// enough frames behind it, from the 7x7 same-key neighbourhood elsewhere — a block stages one luminance and the key of its 32x8
// tile and a 3-texel halo in LDS, so lum is computed once per texel.  It stores the alpha word alone and loads rgb alone: a lane
// never reads a word another lane writes.
//
// The filter is the a-trous body of denoise_device.hpp, instantiated with its second edge-stopping weight, max(lim - d^2, 0),
// lim = sigma^2 * (3x3 prefiltered variance of the centre) + floor: compactly supported, no exp, no per-tap divide, and its
// normalising 1 / lim cancels in num / den.  Steps 1 and 2 stage colour, key and luminance in LDS (36 B per texel, 22.5 KiB at
// step 2); steps >= 4 gather.  The host frame (handles, grid, scratch sequence, pass loop) is tdt_internal.hpp's, shared with
// tdt_denoise.hip.  Every kernel here gives the bits of tests/variance_model.py.
#include <cmath>
#include <string>

#include "tdt_internal.hpp"
#include "denoise_device.hpp"

namespace tdt {

constexpr int kVarRadius = 3;                        // the spatial estimate's window is 7x7

__global__ __launch_bounds__(256) void variance_kernel(float *img, const uint4 *__restrict__ guide, const float4 *__restrict__ moments,
                                                       float min_frames, int w, int h, uint32_t tiles_x) {
  constexpr int TW = kTileW + 2 * kVarRadius, TH = kTileH + 2 * kVarRadius;
  __shared__ float s_lum[TW * TH];
  __shared__ uint4 s_key[TW * TH];
  int x0, y0;
  tile_origin(tiles_x, x0, y0);
  stage_tile<kVarRadius>(guide, w, h, x0, y0, s_key,
                         [&](size_t p) { const float *c = img + 4 * p; return lum(c[0], c[1], c[2]); },   // rgb only: alpha is what this call writes
                         [&](int t, float l) { s_lum[t] = l; });
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

// ---- the variance-guided filter: denoise_device.hpp's one body, VAR, over the staged tile or a gather ----
// steps 1 and 2: the tile and its halo of 2 * S texels through LDS, colour + key + luminance
template <int S>
__global__ __launch_bounds__(256) void denoise_variance_tile_kernel(const float4 *__restrict__ in, const uint4 *__restrict__ guide,
                                                                    float4 *__restrict__ out, float s2, float floor, int w, int h,
                                                                    uint32_t tiles_x) {
  constexpr int N = (kTileW + 4 * S) * (kTileH + 4 * S);
  __shared__ float4 s_col[N];
  __shared__ uint4 s_key[N];
  __shared__ float s_lum[N];
  filter_tile<S, true>(in, guide, out, s2, floor, w, h, tiles_x, s_col, s_key, s_lum);
}

// steps >= 4: every lane gathers its nine distance-1 taps and its 25 taps
__global__ __launch_bounds__(256) void denoise_variance_gather_kernel(const float4 *__restrict__ in, const uint4 *__restrict__ guide,
                                                                      float4 *__restrict__ out, float s2, float floor, int w, int h, int step,
                                                                      uint32_t tiles_x) {
  filter_gather<true>(in, guide, out, s2, floor, w, h, step, tiles_x);
}

}  // namespace tdt

extern "C" {

int tdt_image_variance(tdt_image *img, const tdt_image *guide, const tdt_image *moments, float min_frames, uint32_t flags) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  if (!guide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide image");
  const tdt_image *handles[3] = {img, guide, moments}, *im[3];
  if (int rc = tdt::images_of_context(ctx, handles, 3, "an image belongs to another context")) return rc;
  if (int rc = tdt::images_fit(ctx, handles, 3, 3, im, "image, guide and moments differ in size", "two of the images are one (or share memory)")) return rc;
  if (!(min_frames >= 1.0f)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "min_frames must be at least 1");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  const tdt_image *a = im[0];
  dim3 grid;
  uint32_t tiles_x;
  if (int rc = tdt::image_grid(ctx, a->w, a->h, tdt::kTileW, tdt::kTileH, "image too large", grid, tiles_x)) return rc;
  tdt_ctx *m = tdt::first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  hipLaunchKernelGGL(tdt::variance_kernel, grid, dim3(256), 0, m->stream, a->dev, (const uint4 *)im[1]->dev,
                     im[2] ? (const float4 *)im[2]->dev : nullptr, min_frames, a->w, a->h, tiles_x);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_image_denoise_variance(tdt_image *img, const tdt_image *guide, int passes, float sigma, float floor, uint32_t flags) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  if (!guide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide image");
  const tdt_image *handles[2] = {img, guide}, *im[2];
  if (int rc = tdt::images_of_context(ctx, handles, 2, "guide image belongs to another context")) return rc;
  if (int rc = tdt::images_fit(ctx, handles, 2, 2, im, "image and guide differ in size", "the guide is the image itself (or shares its memory)")) return rc;
  if (passes < 0 || passes > tdt::kMaxPasses) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "passes must be 0..8");
  if (!(sigma > 0.0f) || !std::isfinite(sigma)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "sigma must be positive and finite");
  if (!(floor >= 0.0f) || !std::isfinite(floor)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "floor must be non-negative and finite");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (passes == 0) return TDT_OK;
  const tdt_image *a = im[0];
  const uint4 *G = (const uint4 *)im[1]->dev;
  const float s2 = sigma * sigma;
  return tdt::run_passes(ctx, a, passes, tdt::kTileW, tdt::kTileH,
                         [&](auto tile, int step, dim3 grid, hipStream_t st, const float *from, float *to, uint32_t tiles_x) {
    constexpr int S = decltype(tile)::value;
    const float4 *src = (const float4 *)from;
    float4 *dst = (float4 *)to;
    if constexpr (S == 0) hipLaunchKernelGGL(tdt::denoise_variance_gather_kernel, grid, dim3(256), 0, st, src, G, dst, s2, floor, a->w, a->h, step, tiles_x);
    else hipLaunchKernelGGL(tdt::denoise_variance_tile_kernel<S>, grid, dim3(256), 0, st, src, G, dst, s2, floor, a->w, a->h, tiles_x);
  });
}

}  // extern "C"
