// The image-pass layer on the device (tdt_denoise.hip, tdt_variance.hip, tdt_reproject.hip): the two tiles a block covers, the
// surface key of a guide texel and its comparison, the luminance the variance units measure, the staging of a tile and its halo
// in LDS, and the a-trous filter: the taps' arithmetic once, and a tile and a gather body that each serve the key-only and the
// variance-guided filter.  The operation order that include/tdt_rt.h and the numpy models pin exists here, once; the tap order twice.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "trace_device.hpp"

namespace tdt {

constexpr int kTileW = 32, kTileH = 8;               // pixels of a filter block, one per lane
constexpr uint32_t kRayTile = 16;                    // a block of the guide and reprojection kernels covers a 16x16 tile: neighbouring rays
                                                     // walk the same cells, and the old frame's texels they ask for lie close together

// words 0, 1, 2 of a guide texel; w = 1 marks a texel inside the image (outside: all four zero, which matches no centre)
TDT_DEV uint4 key_of(const uint4 g) { return make_uint4(g.x, g.y, g.z, 1u); }
TDT_DEV bool same_key(const uint4 a, const uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

TDT_DEV void tile_origin(uint32_t tiles_x, int &x0, int &y0) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  x0 = (int)tx * kTileW; y0 = (int)ty * kTileH;
}
// this lane's pixel of the block's 16x16 tile
TDT_DEV void ray_tile_pixel(uint32_t tiles_x, int &x, int &y) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  x = (int)(tx * kRayTile + (threadIdx.x & (kRayTile - 1))); y = (int)(ty * kRayTile + threadIdx.x / kRayTile);
}

// three multiplies and two adds, unfused (the build's parity flags)
TDT_DEV float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The block's 32x8 tile and a halo of HALO texels into LDS.  Texel t of the staged rectangle, kTileW + 2 * HALO wide, gets
// store(t, load(p)) and key[t] = the key of guide[p] where it lies inside the image (p: its index there), store(t, zero) and the
// all-zero key outside.  Ends with the block's barrier.
template <int HALO, class Load, class Store>
TDT_DEV void stage_tile(const uint4 *__restrict__ guide, int w, int h, int x0, int y0, uint4 *key, Load load, Store store) {
  constexpr int TW = kTileW + 2 * HALO, TH = kTileH + 2 * HALO;
  for (int t = (int)threadIdx.x; t < TW * TH; t += 256) {
    const int ly = t / TW, lx = t - ly * TW;
    const int gx = x0 - HALO + lx, gy = y0 - HALO + ly;
    decltype(load((size_t)0)) v{};
    uint4 k = make_uint4(0u, 0u, 0u, 0u);
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const size_t p = (size_t)gy * (size_t)w + (size_t)gx;
      v = load(p); k = key_of(guide[p]);
    }
    store(t, v); key[t] = k;
  }
  __syncthreads();
}

// ---- the a-trous filter ----
// Two bodies, one over the block's staged tile and one that gathers, each both the key-only (VAR false) and the variance-guided
// filter; they share the taps' arithmetic and the centre's rules below.  (One body over a tap source was tried: the tile kernels
// came out instruction for instruction, the gather's bounds branches did not, in any of six forms, and its passes measured slower.)
struct FilterSums { float r, g, b, den, vnum; };
// One tap of the centre's key, colour c and luminance l.  Key-only: w = k[j] * k[i] (exact), the sums grow by an unfused multiply,
// then an add.  VAR: kept when d2 < lim (NaN fails), d = l - the centre's lP; w = (k[j] * k[i]) * (lim - d2), every operation
// rounded on its own, and w^2 * the tap's variance (its alpha) is summed too.
template <bool VAR> TDT_DEV void add_tap(FilterSums &s, int j, int i, const float4 c, float l, float lP, float lim) {
  const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  float w = k[j] * k[i];
  if (VAR) {
    const float d = l - lP;
    const float d2 = d * d;
    if (!(d2 < lim)) return;
    w = w * (lim - d2);
  }
  s.r = s.r + w * c.x; s.g = s.g + w * c.y; s.b = s.b + w * c.z;
  s.den = s.den + w;
  if (VAR) s.vnum = s.vnum + (w * w) * c.w;
}
// alpha: the centre's (key-only), sum(w^2 * variance) / den^2 (VAR)
template <bool VAR> TDT_DEV float4 finish(const FilterSums &s, const float4 centre) {
  return make_float4(s.r / s.den, s.g / s.den, s.b / s.den, VAR ? s.vnum / (s.den * s.den) : centre.w);
}
// one same-key tap of the 3x3 prefilter of the variance a, g = {1/4, 1/2, 1/4}
TDT_DEV void add_prefilter_tap(float &gnum, float &gden, int j, int i, float a) {
  const float g[3] = {0.25f, 0.5f, 0.25f};
  const float wg = g[j] * g[i];
  gnum = gnum + wg * a; gden = gden + wg;
}
// VAR: the centre's limit from its prefiltered variance; a centre whose limit is not usable keeps its colour
TDT_DEV float tap_limit(float gnum, float gden, float s2, float floor) { return s2 * (gnum / gden) + floor; }
TDT_DEV bool usable(float lim) { return lim > 0.f && lim < INFINITY; }

// steps 1 and 2: the tile and its halo of 2 * S texels through the block's LDS arrays (s_col, s_key and, VAR, s_lum: (kTileW +
// 4 * S) * (kTileH + 4 * S) texels each; the distance-1 taps of the prefilter lie inside the halo).  A texel outside the image
// carries the all-zero key, which matches no centre, so no tap needs a bounds test.
template <int S, bool VAR>
TDT_DEV void filter_tile(const float4 *__restrict__ in, const uint4 *__restrict__ guide, float4 *__restrict__ out, float s2, float floor, int w,
                         int h, uint32_t tiles_x, float4 *s_col, uint4 *s_key, float *s_lum) {
  constexpr int TW = kTileW + 4 * S;
  int x0, y0;
  tile_origin(tiles_x, x0, y0);
  stage_tile<2 * S>(guide, w, h, x0, y0, s_key, [&](size_t p) { return in[p]; },
                    [&](int t, const float4 c) { s_col[t] = c; if (VAR) s_lum[t] = lum(c.x, c.y, c.z); });
  const int lx = (int)(threadIdx.x % kTileW), ly = (int)(threadIdx.x / kTileW);
  const int x = x0 + lx, y = y0 + ly;
  if (x >= w || y >= h) return;
  const int centre = (ly + 2 * S) * TW + lx + 2 * S;
  const uint4 ck = s_key[centre];
  float4 o = s_col[centre];
  if (ck.x != 0u) {
    float lim = 0.f, lP = 0.f;
    bool go = true;
    if (VAR) {
      float gnum = 0.f, gden = 0.f;
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const int t = centre + (j - 1) * TW + (i - 1);
          if (same_key(s_key[t], ck)) add_prefilter_tap(gnum, gden, j, i, s_col[t].w);
        }
      lim = tap_limit(gnum, gden, s2, floor);
      go = usable(lim);
      if (go) lP = s_lum[centre];
    }
    if (go) {
      FilterSums s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 5; j++)
#pragma unroll
        for (int i = 0; i < 5; i++) {
          const int t = centre + (j - 2) * S * TW + (i - 2) * S;
          if (same_key(s_key[t], ck)) add_tap<VAR>(s, j, i, s_col[t], VAR ? s_lum[t] : 0.f, lP, lim);
        }
      o = finish<VAR>(s, o);
    }
  }
  out[(size_t)y * (size_t)w + (size_t)x] = o;
}

// steps >= 4, where the taps of neighbouring lanes no longer overlap: every lane gathers its 25 taps (VAR: and its nine
// distance-1 taps) from the images, each behind a bounds test
template <bool VAR>
TDT_DEV void filter_gather(const float4 *__restrict__ in, const uint4 *__restrict__ guide, float4 *__restrict__ out, float s2, float floor, int w,
                           int h, int step, uint32_t tiles_x) {
  int x0, y0;
  tile_origin(tiles_x, x0, y0);
  const int x = x0 + (int)(threadIdx.x % kTileW), y = y0 + (int)(threadIdx.x / kTileW);
  if (x >= w || y >= h) return;
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const uint4 ck = key_of(guide[p]);
  const float4 cc = in[p];
  float4 o = cc;
  if (ck.x != 0u) {
    float lim = 0.f, lP = 0.f;
    bool go = true;
    if (VAR) {
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
      lim = tap_limit(gnum, gden, s2, floor);
      go = usable(lim);
      if (go) lP = lum(cc.x, cc.y, cc.z);
    }
    if (go) {
      FilterSums s = {0.f, 0.f, 0.f, 0.f, 0.f};
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
            add_tap<VAR>(s, j, i, c, VAR ? lum(c.x, c.y, c.z) : 0.f, lP, lim);
          }
        }
      }
      o = finish<VAR>(s, cc);
    }
  }
  out[p] = o;
}

}  // namespace tdt
