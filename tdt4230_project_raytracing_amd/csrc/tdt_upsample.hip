// Guide-keyed upsampling (include/tdt_rt.h, tdt_image_upsample / tdt_debug_upsample_counts).
//
// One lane per pixel of the full-resolution image: the sums of a frame traced at reduced resolution are spread over the full
// frame, and only texels whose guide key (kind, material, plane) equals the full-resolution pixel's may contribute.  A voxel face is
// an axis-aligned plane, so an equal key means "the low-resolution ray saw this face" with no tolerance: radiance never crosses a
// face edge.  The mapping between the two grids is exact integer arithmetic, the arithmetic and its order are the header's, so a
// numpy model gives the same bits.  The host frame (handles, sizes, aliasing, grid) is tdt_internal.hpp's.
//
// The kernel is a gather bound by memory: 16 B read and 16 B written per pixel at home, and 32 B per matching tap gathered from
// the low-resolution pair.  A block covers the guide kernel's 16x16 tile (denoise_device.hpp), so the source texels its lanes ask
// for lie together: at scale 2 a block's taps fall in a 9x9 patch, read four times over from L1 / L2.
#include <string>
#include <vector>

#include "tdt_internal.hpp"
#include "denoise_device.hpp"

namespace tdt {

constexpr int kMaxUpsampleSide = 32768;              // x * (w - 1) < 2^30 then: the products below fit

// One axis of the mapping: pixel x of a side of D + 1 pixels lies at x * last / D of a side of last + 1 texels.
// n / D for every n <= D * D < 2^30 as (n * magic) >> 45, magic = ceil(2^45 / D): with e = magic * D - 2^45 < D the floor is exact
// while n * e < 2^45, and n * magic <= D * 2^45 + D * D fits 64 bits.  D == 0 (a side of one pixel): magic = 0 and fd = 1, so
// that i0 = 0 and f = 0 / 1.
struct UpsampleAxis {
  unsigned long long magic;
  uint32_t d;                                        // D = the full side - 1
  uint32_t last;                                     // the low side - 1
  float fd;                                          // (float)D, exact; 1 when D == 0
};

struct UpsampleArgs {
  UpsampleAxis ax, ay;
  int W, H, w;
  uint32_t tiles_x;
};

constexpr int kUpsampleShift = 45;

// The counts live in kCountSlots groups of four words, each group on a 128-byte line of its own; block b adds into group
// b % kCountSlots and tdt_debug_upsample_counts sums the groups.  Global atomics execute at the memory side, one after the other
// per address: with one group, every block of a launch queued on the same line.  (TDT_UPSAMPLE_COUNT_SLOTS=1 builds that form for
// the A/B of profiles/upsample_counts_ab_mi355x.txt.)
#ifndef TDT_UPSAMPLE_COUNT_SLOTS
#define TDT_UPSAMPLE_COUNT_SLOTS 64
#endif
constexpr uint32_t kCountSlots = TDT_UPSAMPLE_COUNT_SLOTS, kCountStride = 16;   // (words of 8 bytes between two groups)
static_assert((kCountSlots & (kCountSlots - 1)) == 0, "blocks pick their group with a mask");
constexpr size_t kCountBytes = (size_t)kCountSlots * kCountStride * sizeof(unsigned long long);

// A guide texel as one 16-byte load.  Only three of its words are the key, and left alone the compiler narrows the load and splits
// it in two; the empty statement keeps the fourth word live.
TDT_DEV uint4 guide_texel(const uint4 *p) {
  uint4 g = *p;
  asm volatile("" : "+v"(g.w));
  return g;
}

// i0, i1, the nearest texel and the fraction of coordinate c along axis a
TDT_DEV void upsample_map(const UpsampleAxis &a, uint32_t c, int &i0, int &i1, int &in, float &f) {
  const uint32_t n = c * a.last;
  const uint32_t q = (uint32_t)(((unsigned long long)n * a.magic) >> kUpsampleShift);
  const uint32_t r = n - q * a.d;
  i0 = (int)q;
  i1 = (int)(q + 1u < a.last ? q + 1u : a.last);
  in = 2u * r < a.d ? i0 : i1;
  f = (float)r / a.fd;
}

__global__ __launch_bounds__(256) void upsample_kernel(const UpsampleArgs A, const uint4 *__restrict__ dst_guide, const uint4 *__restrict__ src_guide,
                                                       const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                       unsigned long long *__restrict__ counts) {
  __shared__ uint32_t s_count[4];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0u;
  __syncthreads();
  int x, y;
  ray_tile_pixel(A.tiles_x, x, y);
  uint32_t cls = 0u;                                 // 0 = outside the image, 1 = validated bilinear, 2 = the ring, 3 = a hole
  if (x < A.W && y < A.H) {
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const uint4 g = guide_texel(dst_guide + p);
    int i[2], j[2], in, jn;
    float fx, fy;
    upsample_map(A.ax, (uint32_t)x, i[0], i[1], in, fx);
    upsample_map(A.ay, (uint32_t)y, j[0], j[1], jn, fy);
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
    float4 num = make_float4(0.f, 0.f, 0.f, 0.f);
    float den = 0.f;
    // stage 1: the four taps of the bilinear footprint, those of this pixel's surface only
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int a = 0; a < 2; a++) {
        const float wt = wy[b] * wx[a];
        if (!(wt > 0.f)) continue;
        const size_t q = (size_t)j[b] * (size_t)A.w + (size_t)i[a];
        const uint4 k = guide_texel(src_guide + q);
        if (k.x != g.x || k.y != g.y || k.z != g.z) continue;
        const float4 c = src[q];
        num.x = num.x + wt * c.x; num.y = num.y + wt * c.y; num.z = num.z + wt * c.z; num.w = num.w + wt * c.w;
        den = den + wt;
      }
    float4 o;
    if (den > 0.f) {
      o = make_float4(num.x / den, num.y / den, num.z / den, num.w / den);
      cls = 1u;
    } else {
      // stage 2, for the lanes whose footprint missed their surface: the plain mean of the same-key texels of the 4x4 ring
      float K = 0.f;
      const int h = (int)A.ay.last + 1;
#pragma unroll 1
      for (int qy = j[0] - 1; qy <= j[0] + 2; qy++) {
        if (qy < 0 || qy >= h) continue;
#pragma unroll 1
        for (int qx = i[0] - 1; qx <= i[0] + 2; qx++) {
          if (qx < 0 || qx >= A.w) continue;
          const size_t q = (size_t)qy * (size_t)A.w + (size_t)qx;
          const uint4 k = guide_texel(src_guide + q);
          if (k.x != g.x || k.y != g.y || k.z != g.z) continue;
          const float4 c = src[q];
          num.x = num.x + c.x; num.y = num.y + c.y; num.z = num.z + c.z; num.w = num.w + c.w;
          K = K + 1.0f;
        }
      }
      if (K > 0.f) {
        o = make_float4(num.x / K, num.y / K, num.z / K, num.w / K);
        cls = 2u;
      } else {                                       // stage 3: nothing nearby saw this surface; the nearest texel, as it is
        o = src[(size_t)jn * (size_t)A.w + (size_t)in];
        cls = 3u;
      }
    }
    dst[p] = o;
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
    atomicAdd(&counts[(blockIdx.x & (kCountSlots - 1u)) * kCountStride + threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

namespace {

UpsampleAxis upsample_axis(int full, int low) {
  UpsampleAxis a;
  a.d = (uint32_t)(full - 1); a.last = (uint32_t)(low - 1);
  a.magic = a.d ? ((1ull << kUpsampleShift) + a.d - 1ull) / a.d : 0ull;
  a.fd = a.d ? (float)a.d : 1.0f;
  return a;
}

}  // namespace

void upsample_counts_destroy(tdt_ctx *ctx) {
  if (ctx->upsample_counts) (void)hipFree(ctx->upsample_counts);
  ctx->upsample_counts = nullptr;
}

}  // namespace tdt

extern "C" {

int tdt_image_upsample(tdt_image *dst, const tdt_image *dst_guide, const tdt_image *src, const tdt_image *src_guide, uint32_t flags) {
  if (!dst) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = dst->ctx;
  if (!dst_guide || !src || !src_guide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide or source image");
  constexpr int N = 4;
  const tdt_image *handles[N] = {dst, dst_guide, src, src_guide}, *im[N];
  if (int rc = tdt::images_of_context(ctx, handles, N, "an image belongs to another context")) return rc;
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (int rc = tdt::images_fit(ctx, handles, N, 2, im, "the image and its guide differ in size", "two of the images are one (or share memory)"))
    return rc;
  const tdt_image *d = im[0], *dg = im[1], *s = im[2], *sg = im[3];
  if (s->w != sg->w || s->h != sg->h) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the source and its guide differ in size");
  if (s->w > d->w || s->h > d->h) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the source is wider or taller than the image");
  if (d->w > tdt::kMaxUpsampleSide || d->h > tdt::kMaxUpsampleSide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "a side above 32768");
  tdt::UpsampleArgs A;
  A.ax = tdt::upsample_axis(d->w, s->w); A.ay = tdt::upsample_axis(d->h, s->h);
  A.W = d->w; A.H = d->h; A.w = s->w;
  dim3 grid;
  if (int rc = tdt::image_grid(ctx, d->w, d->h, tdt::kRayTile, tdt::kRayTile, "image too large", grid, A.tiles_x)) return rc;
  tdt_ctx *m = tdt::first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  if (!m->upsample_counts) {
    const hipError_t e = hipMalloc((void **)&m->upsample_counts, tdt::kCountBytes);
    if (e != hipSuccess) { m->upsample_counts = nullptr; return tdt::hip_fail(ctx, e, "hipMalloc (upsample counts)"); }
  }
  TDT_HIP(ctx, hipMemsetAsync(m->upsample_counts, 0, tdt::kCountBytes, m->stream));
  hipLaunchKernelGGL(tdt::upsample_kernel, grid, dim3(256), 0, m->stream, A, (const uint4 *)dg->dev, (const uint4 *)sg->dev, (const float4 *)s->dev,
                     (float4 *)d->dev, m->upsample_counts);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_debug_upsample_counts(tdt_ctx *ctx, uint64_t out[4]) {
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null counts");
  tdt_ctx *m = tdt::first_member(ctx);
  std::vector<unsigned long long> host((size_t)tdt::kCountSlots * tdt::kCountStride, 0ull);
  TDT_HIP(ctx, hipSetDevice(m->device));
  if (m->upsample_counts) TDT_HIP(ctx, hipMemcpyAsync(host.data(), m->upsample_counts, tdt::kCountBytes, hipMemcpyDeviceToHost, m->stream));
  TDT_HIP(ctx, hipStreamSynchronize(m->stream));
  for (int i = 0; i < 4; i++) {
    out[i] = 0;
    for (uint32_t s = 0; s < tdt::kCountSlots; s++) out[i] += host[(size_t)s * tdt::kCountStride + i];
  }
  return TDT_OK;
}

}  // extern "C"
