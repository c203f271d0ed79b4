// The sampling controller (include/tdt_rt.h, tdt_image_adapt / tdt_debug_adapt_counts / tdt_image_adapt_mean).
//
// Adaptive sampling in two halves.  The trace half is tdt_dispatch_accumulate_masked (tdt_rt.hip): a batch of samples for the
// pixels whose mask texel is live.  This unit is the other half: after a batch it folds the batch's mean luminance into a per-pixel
// state texel (L, m2, n, w) and decides from the variance of the batch means which pixels have settled.  A stopped pixel carries
// w < 0, so the state image IS the next batch's mask and nothing is converted in between.
//
// With a guide a pixel only stops when every same-key texel of its 3x3 neighbourhood passes too: a pixel whose two batches happened
// to agree does not stop in the middle of a face that is still noisy.  The block stages (key, test) of its 32x8 tile and a halo of
// one texel in LDS through denoise_device.hpp's stage_tile, so a texel's update is evaluated once per block that sees it and the
// neighbourhood costs no memory traffic.  state_in and state_out are distinct images: no lane reads a word another writes.
// Both kernels are bound by memory (adapt: 32 B or 48 B read and 16 B written per pixel; adapt_mean: 32 B read, 16 B written).
// The arithmetic and its order are the header's, so tests/adaptive_model.py gives the same bits.
#include <cmath>
#include <string>
#include <vector>

#include "tdt_internal.hpp"
#include "denoise_device.hpp"

namespace tdt {

struct AdaptArgs {
  float kf;                                          // (float)spp_count
  float tolerance, floor, min_samples, max_samples;  // the limits as floats (exact: both are below 2^24)
  int w, h;
  uint32_t tiles_x;
};

// The counts live in kAdaptCountSlots groups of four words, each on a 128-byte line of its own, as tdt_upsample.hip's do: block b
// adds into group b % kAdaptCountSlots and tdt_debug_adapt_counts sums the groups.  (With one group every block of a launch queued
// on the same line at the memory side: measured at 1280x720, 0.049 ms without a guide and 0.056 ms with one; in 64 groups 0.010 and
// 0.021 ms.)
constexpr uint32_t kAdaptCountSlots = 64, kAdaptCountStride = 16;      // (words of 8 bytes between two groups)
constexpr size_t kAdaptCountBytes = (size_t)kAdaptCountSlots * kAdaptCountStride * sizeof(unsigned long long);

enum : uint32_t { ADAPT_LIVE = 1u, ADAPT_PASS = 2u, ADAPT_CAPPED = 4u };

// The update of one texel: out = the state after the batch, with w still positive (the caller negates it when the pixel stops).
// Returns ADAPT_PASS alone for a pixel that had stopped before (out = st), else ADAPT_LIVE with ADAPT_CAPPED and ADAPT_PASS as the
// header's tests say (a capped pixel passes).
TDT_DEV uint32_t adapt_update(const AdaptArgs &A, const float4 sums, const float4 st, float4 &out) {
  out = st;
  if (!(st.w >= 0.0f)) return ADAPT_PASS;
  const float Lc = lum(sums.x, sums.y, sums.z);
  const float lb = (Lc - st.x) / A.kf;
  const float m2 = st.y + lb * lb;
  const float n = st.z + 1.0f;
  const float s = st.w + A.kf;
  const float mean = Lc / s;
  const float v = m2 / n - mean * mean;
  const float var = v < 0.0f ? 0.0f : v;             // (a NaN stays a NaN and fails the comparison below)
  const float err2 = var / n;
  const float mx = mean > A.floor ? mean : A.floor;
  const float thr = A.tolerance * mx;
  const float thr2 = thr * thr;
  out = make_float4(Lc, m2, n, s);
  if (s >= A.max_samples) return ADAPT_LIVE | ADAPT_CAPPED | ADAPT_PASS;
  const bool own = s >= A.min_samples && n >= 2.0f && err2 <= thr2;
  return ADAPT_LIVE | (own ? ADAPT_PASS : 0u);
}

// one lane per pixel of a 32x8 tile; GUIDE: the stop also needs every same-key texel of the 3x3 neighbourhood to pass
template <bool GUIDE>
__global__ __launch_bounds__(256) void adapt_kernel(const AdaptArgs A, const float4 *__restrict__ sums, const uint4 *__restrict__ guide,
                                                    const float4 *__restrict__ state_in, float4 *__restrict__ state_out,
                                                    unsigned long long *__restrict__ counts) {
  constexpr int TW = kTileW + 2, TH = kTileH + 2;
  __shared__ uint32_t s_count[4];
  __shared__ uint4 s_key[GUIDE ? TW * TH : 1];
  __shared__ uint32_t s_test[GUIDE ? TW * TH : 1];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0u;
  int x0, y0;
  tile_origin(A.tiles_x, x0, y0);
  if (GUIDE) {
    stage_tile<1>(guide, A.w, A.h, x0, y0, s_key,
                  [&](size_t p) { float4 o; return adapt_update(A, sums[p], state_in[p], o); },
                  [&](int t, uint32_t f) { s_test[t] = f; });
  } else {
    __syncthreads();
  }
  const int lx = (int)(threadIdx.x % kTileW), ly = (int)(threadIdx.x / kTileW);
  const int x = x0 + lx, y = y0 + ly;
  uint32_t cls = 0u;                                 // 0 = outside the image or stopped before, 1 = stopped by the tolerance, 2 = by the cap, 3 = still live
  if (x < A.w && y < A.h) {
    const size_t p = (size_t)y * (size_t)A.w + (size_t)x;
    float4 o;
    const uint32_t f = adapt_update(A, sums[p], state_in[p], o);
    // the same-key texels of the 3x3 neighbourhood that do not pass (the centre among them), counted by every lane: no branch
    // depends on the lane's own test
    uint32_t waiting = (f & ADAPT_PASS) ? 0u : 1u;
    if (GUIDE) {
      const int centre = (ly + 1) * TW + lx + 1;
      const uint4 ck = s_key[centre];
      waiting = 0u;
#pragma unroll
      for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++) {
          const int t = centre + j * TW + i;
          waiting += (same_key(s_key[t], ck) && !(s_test[t] & ADAPT_PASS)) ? 1u : 0u;
        }
    }
    const bool live = (f & ADAPT_LIVE) != 0u, capped = (f & ADAPT_CAPPED) != 0u;
    const bool stop = live && (capped || waiting == 0u);
    o.w = stop ? -o.w : o.w;
    cls = !live ? 0u : (!stop ? 3u : (capped ? 2u : 1u));
    state_out[p] = o;
  }
  // the block's counts: one LDS add per wave and counter, then one global add per counter into the block's group
  const unsigned long long m0 = __ballot(cls != 0u), m1 = __ballot(cls == 1u), m2 = __ballot(cls == 2u), m3 = __ballot(cls == 3u);
  if ((threadIdx.x & 63u) == 0u) {
    if (m0) atomicAdd(&s_count[0], (uint32_t)__popcll(m0));
    if (m1) atomicAdd(&s_count[1], (uint32_t)__popcll(m1));
    if (m2) atomicAdd(&s_count[2], (uint32_t)__popcll(m2));
    if (m3) atomicAdd(&s_count[3], (uint32_t)__popcll(m3));
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_count[threadIdx.x])
    atomicAdd(&counts[(blockIdx.x & (kAdaptCountSlots - 1u)) * kAdaptCountStride + threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

// the means and the variance of the mean luminance from the sums and the final state; a pixel with no samples is left alone
__global__ __launch_bounds__(256) void adapt_mean_kernel(float4 *img, const float4 *__restrict__ state, int w, int h, uint32_t tiles_x) {
  int x0, y0;
  tile_origin(tiles_x, x0, y0);
  const int x = x0 + (int)(threadIdx.x % kTileW), y = y0 + (int)(threadIdx.x / kTileW);
  if (x >= w || y >= h) return;
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const float4 st = state[p];
  const float aw = __builtin_fabsf(st.w);
  if (aw == 0.0f) return;
  const float4 c = img[p];
  float a = 0.0f;
  if (st.z >= 2.0f) {
    const float mean = st.x / aw;
    const float v = st.y / st.z - mean * mean;
    a = (v > 0.0f ? v : 0.0f) / st.z;
  }
  img[p] = make_float4(c.x / aw, c.y / aw, c.z / aw, a);
}

void adapt_counts_destroy(tdt_ctx *ctx) {
  if (ctx->adapt_counts) (void)hipFree(ctx->adapt_counts);
  ctx->adapt_counts = nullptr;
}

}  // namespace tdt

extern "C" {

int tdt_image_adapt(const tdt_image *sums, const tdt_image *guide, const tdt_image *state_in, tdt_image *state_out, int spp_count,
                    const tdt_adapt *a, uint32_t flags) {
  if (!state_out) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = state_out->ctx;
  if (!sums || !state_in) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null sums or state image");
  if (!a) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_adapt");
  constexpr int N = 4;
  const tdt_image *handles[N] = {state_out, state_in, sums, guide}, *im[N];
  if (int rc = tdt::images_of_context(ctx, handles, N, "an image belongs to another context")) return rc;
  if (ctx->multi) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "tdt_image_adapt works on a single-device context");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (spp_count < 1 || spp_count > (1 << 24)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "spp_count must be 1..2^24");
  if (!(a->tolerance >= 0.0f) || !std::isfinite(a->tolerance)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "tolerance must be non-negative and finite");
  if (!(a->floor >= 0.0f) || !std::isfinite(a->floor)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "floor must be non-negative and finite");
  if (a->min_samples < 0 || a->min_samples > (1 << 24)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "min_samples must be 0..2^24");
  if (a->max_samples < 1 || a->max_samples > (1 << 24)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "max_samples must be 1..2^24");
  if (int rc = tdt::images_fit(ctx, handles, N, N, im, "sums, guide and the two state images differ in size", "two of the images are one (or share memory)"))
    return rc;
  tdt::AdaptArgs A;
  A.kf = (float)spp_count; A.tolerance = a->tolerance; A.floor = a->floor;
  A.min_samples = (float)a->min_samples; A.max_samples = (float)a->max_samples;
  A.w = im[0]->w; A.h = im[0]->h;
  dim3 grid;
  if (int rc = tdt::image_grid(ctx, A.w, A.h, tdt::kTileW, tdt::kTileH, "image too large", grid, A.tiles_x)) return rc;
  TDT_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->adapt_counts) {
    const hipError_t e = hipMalloc((void **)&ctx->adapt_counts, tdt::kAdaptCountBytes);
    if (e != hipSuccess) { ctx->adapt_counts = nullptr; return tdt::hip_fail(ctx, e, "hipMalloc (adapt counts)"); }
  }
  TDT_HIP(ctx, hipMemsetAsync(ctx->adapt_counts, 0, tdt::kAdaptCountBytes, ctx->stream));
  const float4 *S = (const float4 *)im[2]->dev, *SI = (const float4 *)im[1]->dev;
  float4 *SO = (float4 *)im[0]->dev;
  if (im[3]) hipLaunchKernelGGL(tdt::adapt_kernel<true>, grid, dim3(256), 0, ctx->stream, A, S, (const uint4 *)im[3]->dev, SI, SO, ctx->adapt_counts);
  else hipLaunchKernelGGL(tdt::adapt_kernel<false>, grid, dim3(256), 0, ctx->stream, A, S, (const uint4 *)nullptr, SI, SO, ctx->adapt_counts);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_debug_adapt_counts(tdt_ctx *ctx, uint64_t out[4]) {
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null counts");
  if (ctx->multi) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "tdt_debug_adapt_counts works on a single-device context");
  std::vector<unsigned long long> host((size_t)tdt::kAdaptCountSlots * tdt::kAdaptCountStride, 0ull);
  TDT_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->adapt_counts) TDT_HIP(ctx, hipMemcpyAsync(host.data(), ctx->adapt_counts, tdt::kAdaptCountBytes, hipMemcpyDeviceToHost, ctx->stream));
  TDT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 4; i++) {
    out[i] = 0;
    for (uint32_t k = 0; k < tdt::kAdaptCountSlots; k++) out[i] += host[(size_t)k * tdt::kAdaptCountStride + i];
  }
  return TDT_OK;
}

int tdt_image_adapt_mean(tdt_image *img, const tdt_image *state, uint32_t flags) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  if (!state) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null state image");
  const tdt_image *handles[2] = {img, state}, *im[2];
  if (int rc = tdt::images_of_context(ctx, handles, 2, "the state image belongs to another context")) return rc;
  if (ctx->multi) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "tdt_image_adapt_mean works on a single-device context");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (int rc = tdt::images_fit(ctx, handles, 2, 2, im, "image and state differ in size", "the state is the image itself (or shares its memory)")) return rc;
  dim3 grid;
  uint32_t tiles_x;
  if (int rc = tdt::image_grid(ctx, im[0]->w, im[0]->h, tdt::kTileW, tdt::kTileH, "image too large", grid, tiles_x)) return rc;
  TDT_HIP(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(tdt::adapt_mean_kernel, grid, dim3(256), 0, ctx->stream, (float4 *)im[0]->dev, (const float4 *)im[1]->dev, im[0]->w, im[0]->h, tiles_x);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

}  // extern "C"
