// The device side both reprojection kernels of tdt_reproject.hip share (reproject_kernel, reproject_moments_kernel): the per-call
// arguments and the one body, so that Q (view_project, which tdt_screen.hip calls too) and the FOUND predicate exist once.  The
// block's tile is denoise_device.hpp's 16x16.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "tdt_internal.hpp"
#include "trace_params.h"
#include "trace_device.hpp"
#include "denoise_device.hpp"

namespace tdt {

// Q, the projection of the header (tdt_image_reproject; tdt_screen.hip maps voxels through it too): d = the world point minus the
// view's origin; nw and the pixel coordinates (fx, fy) before the cast.  Every operation rounded, none fused; a caller only compares
// fx and fy (a NaN fails) before it casts them.
TDT_DEV void view_project(const ViewRows &V, float dx, float dy, float dz, float &nw, float &fx, float &fy) {
  const float nu = (V.ru[2] * dz + V.ru[1] * dy) + V.ru[0] * dx;
  const float nv = (V.rv[2] * dz + V.rv[1] * dy) + V.rv[0] * dx;
  nw = (V.rw[2] * dz + V.rw[1] * dy) + V.rw[0] * dx;
  fx = (nu / nw) * V.sx; fy = (nv / nw) * V.sy;
}

struct ReprojectArgs {
  ViewRows view;                                     // the earlier view (tdt_internal.hpp, view_rows)
  float fpw, fph;                                    // (float) sizes of the earlier images
  int pw;                                            // their row length
  int has_prev;
  float fspp, max_samples;
};

// The one body of both kernels.  MOMENTS adds the moments image (tdt_image_reproject_moments): the frame's luminance and its
// square join the moments of the texel the history came from; everything else, Q and the FOUND predicate included, is this code.
template <bool MOMENTS>
TDT_DEV void reproject_body(const TraceParams &P, int sample, const ReprojectArgs &A, const uint4 *__restrict__ guide, const float4 *sums,
                            const uint4 *__restrict__ prev_guide, const float4 *__restrict__ prev_hist, float4 *__restrict__ hist_out,
                            float4 *mean_out, int w, int h, uint32_t tiles_x, unsigned long long *__restrict__ counts,
                            const float4 *__restrict__ prev_moments, float4 *__restrict__ moments_out, float mf) {
  __shared__ uint32_t s_count[4];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0u;
  __syncthreads();
  int x, y;
  ray_tile_pixel(tiles_x, x, y);
  // what became of this lane's pixel: 0 = outside the image or not keyed, 1 = found, 2 = rejected by key or hn, 3 = by nw or off-screen
  uint32_t fate = 0u;
  bool keyed = false;
  if (x < w && y < h) {
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    const uint4 g = guide[p];
    const float4 s = sums[p];
    float4 o = make_float4(s.x, s.y, s.z, A.fspp);
    float4 mo = make_float4(0.f, 0.f, 1.0f, 0.f);
    if (MOMENTS) {
      const float l = lum(s.x / A.fspp, s.y / A.fspp, s.z / A.fspp);
      mo.x = l; mo.y = l * l;
    }
    keyed = g.x != 0u;
    if (keyed && A.has_prev) {
      const Ray r = primary_ray(P, x, y, sample);
      const float t = __uint_as_float(g.w);
      const float dx = (r.ox + t * r.dx) - A.view.org[0], dy = (r.oy + t * r.dy) - A.view.org[1], dz = (r.oz + t * r.dz) - A.view.org[2];
      float nw, fx, fy;
      view_project(A.view, dx, dy, dz, nw, fx, fy);
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
            if (MOMENTS) {
              float4 hm = prev_moments[q];
              if (hm.z > 0.f) {
                if (hm.z > mf) {
                  const float sc = mf / hm.z;
                  hm.x = hm.x * sc; hm.y = hm.y * sc; hm.z = mf;
                }
                mo = make_float4(mo.x + hm.x, mo.y + hm.y, 1.0f + hm.z, 0.f);
              }
            }
          }
        }
      }
    }
    hist_out[p] = o;
    if (MOMENTS) moments_out[p] = mo;
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

}  // namespace tdt
