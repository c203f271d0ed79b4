// First-hit guide images and the edge-stopping denoiser (include/tdt_rt.h, tdt_dispatch_guide / tdt_image_denoise).
//
// Guide: one lane per texel traces the primary ray of its pixel through query_first_hit (query_device.hpp: the traversal the
// query unit runs) and stores four words of the record — the key (kind, material, plane) that says "same surface" exactly,
// and the depth.  Voxel faces are axis-aligned, so the key needs no tolerance.
//
// Filter: an a-trous wavelet filter, B3 kernel, whose only edge-stopping function is equality of the key.  The tap order and the
// operation order are fixed per pixel (tdt_rt.h), so every kernel below gives the same bits: for steps 1 and 2 a block stages its
// 32x8 tile and the 2*step halo in LDS — colour and key, 32 B per texel, read once from memory instead of 25 times — and for
// steps >= 4, where the taps of neighbouring lanes no longer overlap, each lane gathers its 25 taps directly.
#include <new>
#include <string>

#include "tdt_internal.hpp"
#include "query_device.hpp"
#include "denoise_device.hpp"

namespace tdt {

constexpr uint32_t kGuideTile = 16;                  // a block traces a 16x16 tile of texels: neighbouring rays walk the same cells

__global__ __launch_bounds__(256) void guide_kernel(const TraceParams P, int sample, int all_materials, uint4 *__restrict__ guide, int gw, int gh,
                                                    uint32_t tiles_x) {
  __shared__ uint16_t s_escape[1];                   // fetch_node's LDS table of zero entries (query_node_source)
  if (threadIdx.x == 0) s_escape[0] = (uint16_t)kPackedEscape;
  __syncthreads();
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = (int)(tx * kGuideTile + (threadIdx.x & (kGuideTile - 1))), y = (int)(ty * kGuideTile + threadIdx.x / kGuideTile);
  if (x >= gw || y >= gh) return;
  const NodeSource ns = query_node_source(P, s_escape);
  const Ray r = primary_ray(P, x, y, sample);
  const QueryRecord q = query_first_hit(P, ns, r);

  const float nx = q.rec.nx, ny = q.rec.ny, nz = q.rec.nz;
  bool keyed = q.status == TDT_RAY_HIT && q.fresh && !(nx == 0.f && ny == 0.f && nz == 0.f);
  if (keyed && !all_materials) {                     // Lambertian only: the type word of entry `material` of slot 1, inside the buffer
    const unsigned long long w = 3ull * q.material;
    keyed = w + 2ull < (unsigned long long)P.materials_dwords && P.materials[w] == 0u;
  }
  uint32_t kind = 0u, plane = 0u;
  if (keyed) {
    const uint32_t sx = nx < 0.f ? 0u : (nx > 0.f ? 2u : 1u), sy = ny < 0.f ? 0u : (ny > 0.f ? 2u : 1u), sz = nz < 0.f ? 0u : (nz > 0.f ? 2u : 1u);
    kind = 1u + (9u * sx + 3u * sy + sz);
    // the first axis whose normal component is not zero carries the face's plane
    const float na = nx != 0.f ? nx : (ny != 0.f ? ny : nz);
    const float ca = nx != 0.f ? q.cmin_x : (ny != 0.f ? q.cmin_y : q.cmin_z);
    plane = __float_as_uint(ca + (na > 0.f ? q.csize : 0.0f));
  }
  guide[(size_t)y * (size_t)gw + (size_t)x] = make_uint4(kind, q.material, plane, __float_as_uint(q.t));
}

// ---- the filter (tile, key_of, same_key, tile_origin: denoise_device.hpp, shared with tdt_variance.hip) ----
struct Sums { float r, g, b, den; };
// one kept tap: w = k[j] * k[i] (exact), unfused multiply, then add (the build's parity flags)
TDT_DEV void add_tap(Sums &s, int j, int i, const float4 c) {
  const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  const float w = k[j] * k[i];
  s.r = s.r + w * c.x; s.g = s.g + w * c.y; s.b = s.b + w * c.z;
  s.den = s.den + w;
}
TDT_DEV float4 finish(const Sums &s, const float4 centre) { return make_float4(s.r / s.den, s.g / s.den, s.b / s.den, centre.w); }

// steps 1 and 2: the tile and its halo of 2 * S texels through LDS
template <int S>
__global__ __launch_bounds__(256) void denoise_tile_kernel(const float4 *__restrict__ in, const uint4 *__restrict__ guide, float4 *__restrict__ out,
                                                           int w, int h, uint32_t tiles_x) {
  constexpr int TW = kTileW + 4 * S, TH = kTileH + 4 * S;
  __shared__ float4 s_col[TW * TH];
  __shared__ uint4 s_key[TW * TH];
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
    s_col[t] = c; s_key[t] = k;
  }
  __syncthreads();
  const int lx = (int)(threadIdx.x % kTileW), ly = (int)(threadIdx.x / kTileW);
  const int x = x0 + lx, y = y0 + ly;
  if (x >= w || y >= h) return;
  const int centre = (ly + 2 * S) * TW + lx + 2 * S;
  const uint4 ck = s_key[centre];
  const float4 cc = s_col[centre];
  float4 o = cc;
  if (ck.x != 0u) {
    Sums s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 5; j++)
#pragma unroll
      for (int i = 0; i < 5; i++) {
        const int t = centre + (j - 2) * S * TW + (i - 2) * S;
        if (same_key(s_key[t], ck)) add_tap(s, j, i, s_col[t]);
      }
    o = finish(s, cc);
  }
  out[(size_t)y * (size_t)w + (size_t)x] = o;
}

// steps >= 4: every lane gathers its own taps
__global__ __launch_bounds__(256) void denoise_gather_kernel(const float4 *__restrict__ in, const uint4 *__restrict__ guide, float4 *__restrict__ out,
                                                             int w, int h, int step, uint32_t tiles_x) {
  int x0, y0;
  tile_origin(tiles_x, x0, y0);
  const int x = x0 + (int)(threadIdx.x % kTileW), y = y0 + (int)(threadIdx.x / kTileW);
  if (x >= w || y >= h) return;
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const uint4 ck = key_of(guide[p]);
  const float4 cc = in[p];
  float4 o = cc;
  if (ck.x != 0u) {
    Sums s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const long long qy = (long long)y + (long long)(j - 2) * step;
#pragma unroll
      for (int i = 0; i < 5; i++) {
        const long long qx = (long long)x + (long long)(i - 2) * step;
        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
        const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
        if (same_key(key_of(guide[q]), ck)) add_tap(s, j, i, in[q]);
      }
    }
    o = finish(s, cc);
  }
  out[p] = o;
}

namespace {

int denoise_scratch(tdt_ctx *front, tdt_ctx *m, size_t bytes, void **out) {
  if (m->denoise_bytes < bytes) {
    TDT_HIP(front, hipStreamSynchronize(m->stream));            // (passes queued earlier may still use the old one)
    denoise_scratch_destroy(m);
    const hipError_t e = hipMalloc(&m->denoise, bytes);
    if (e != hipSuccess) { m->denoise = nullptr; return hip_fail(front, e, "hipMalloc (denoise scratch)"); }
    m->denoise_bytes = bytes;
  }
  *out = m->denoise;
  return TDT_OK;
}

}  // namespace

int denoise_sequence(tdt_ctx *front, tdt_ctx *m, float *img, int w, int h, int passes, float **seq) {
  // The result must end in img.  An even number of passes alternates img -> S1 -> img; an odd number of three or more opens with
  // img -> S1 -> S2 -> img, which leaves an even rest; one pass alone goes to S1 and is copied back (a pass cannot run in place).
  const size_t bytes = (size_t)w * (size_t)h * 16;
  const bool three = (passes & 1) && passes >= 3;
  void *scratch = nullptr;
  if (int rc = denoise_scratch(front, m, three ? 2 * bytes : bytes, &scratch)) return rc;
  float *const I = img, *const S1 = (float *)scratch, *const S2 = (float *)((char *)scratch + bytes);
  int n = 0, rest = passes;
  seq[n++] = I;
  if (three) { seq[n++] = S1; seq[n++] = S2; seq[n++] = I; rest -= 3; }
  for (; rest >= 2; rest -= 2) { seq[n++] = S1; seq[n++] = I; }
  if (rest) seq[n++] = S1;
  return TDT_OK;
}

void denoise_scratch_destroy(tdt_ctx *ctx) {
  if (ctx->denoise) (void)hipFree(ctx->denoise);
  ctx->denoise = nullptr; ctx->denoise_bytes = 0;
}

}  // namespace tdt

extern "C" {

int tdt_dispatch_guide(tdt_compute *c, tdt_image *guide, int sample, uint32_t flags) {
  if (!c) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = c->ctx;
  if (!guide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide image");
  if (c->kind != TDT_PROGRAM_RAYTRACER) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "a guide needs a raytracer program (its camera)");
  if (guide->ctx != ctx) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "guide image belongs to another context");
  if (sample < 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "negative sample index");
  if (flags & ~(uint32_t)TDT_GUIDE_ALL_MATERIALS) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "unknown guide flags");
  if (c->part_rank != 0 || c->part_world != 1)
    return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "a guide is an image, not a tile buffer: the program's partition must be (0, 1)");
  const bool all = (flags & TDT_GUIDE_ALL_MATERIALS) != 0;
  const tdt_compute *cam = c->replicas.empty() ? c : c->replicas[0];     // (a multi-device program: its first member's camera)
  tdt_ctx *m = cam->ctx;
  TraceParams P;
  if (int rc = tdt::query_params(ctx, m, P)) return rc;
  if (!all) {
    const tdt_buffer *mat = m->ssbo[TDT_SLOT_MATERIALS];
    if (!mat) return tdt::fail(ctx, TDT_ERR_INCOMPLETE, "no buffer bound to shader-storage slot 1");
    P.materials = (const uint32_t *)mat->dev;
    P.materials_dwords = (mat->bytes >> 2) > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(mat->bytes >> 2);
  }
  tdt::query_camera(cam, P);
  const tdt_image *g = tdt::device_image(guide);
  const unsigned long long tiles_x = ((unsigned long long)g->w + tdt::kGuideTile - 1) / tdt::kGuideTile,
                           tiles_y = ((unsigned long long)g->h + tdt::kGuideTile - 1) / tdt::kGuideTile;
  if (tiles_x * tiles_y > 0x7FFFFFFFull) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "guide image too large");
  TDT_HIP(ctx, hipSetDevice(m->device));
  hipLaunchKernelGGL(tdt::guide_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, m->stream, P, sample, all ? 1 : 0, (uint4 *)g->dev, g->w, g->h,
                     (uint32_t)tiles_x);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_image_denoise(tdt_image *img, const tdt_image *guide, int passes, uint32_t flags) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  if (!guide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide image");
  if (guide->ctx != ctx) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "guide image belongs to another context");
  const tdt_image *a = tdt::device_image(img), *g = tdt::device_image(guide);
  if (a->w != g->w || a->h != g->h) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "image and guide differ in size");
  const size_t floats = (size_t)a->w * (size_t)a->h * 4;
  if (img == guide || (a->dev < g->dev + floats && g->dev < a->dev + floats))
    return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the guide is the image itself (or shares its memory)");
  if (passes < 0 || passes > tdt::kMaxPasses) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "passes must be 0..8");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (passes == 0) return TDT_OK;
  const unsigned long long tiles_x = ((unsigned long long)a->w + tdt::kTileW - 1) / tdt::kTileW,
                           tiles_y = ((unsigned long long)a->h + tdt::kTileH - 1) / tdt::kTileH;
  if (tiles_x * tiles_y > 0x7FFFFFFFull) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "image too large");
  tdt_ctx *m = tdt::first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  float *seq[tdt::kMaxPasses + 1];
  if (int rc = tdt::denoise_sequence(ctx, m, a->dev, a->w, a->h, passes, seq)) return rc;
  float *const I = seq[0];
  const size_t bytes = (size_t)a->w * (size_t)a->h * 16;
  const dim3 grid((unsigned)(tiles_x * tiles_y)), block(256);
  for (int p = 0; p < passes; p++) {
    const float4 *src = (const float4 *)seq[p];
    float4 *dst = (float4 *)seq[p + 1];
    if (p == 0) hipLaunchKernelGGL(tdt::denoise_tile_kernel<1>, grid, block, 0, m->stream, src, (const uint4 *)g->dev, dst, a->w, a->h, (uint32_t)tiles_x);
    else if (p == 1) hipLaunchKernelGGL(tdt::denoise_tile_kernel<2>, grid, block, 0, m->stream, src, (const uint4 *)g->dev, dst, a->w, a->h, (uint32_t)tiles_x);
    else hipLaunchKernelGGL(tdt::denoise_gather_kernel, grid, block, 0, m->stream, src, (const uint4 *)g->dev, dst, a->w, a->h, 1 << p, (uint32_t)tiles_x);
  }
  TDT_HIP(ctx, hipGetLastError());
  if (seq[passes] != I) TDT_HIP(ctx, hipMemcpyAsync(I, seq[passes], bytes, hipMemcpyDeviceToDevice, m->stream));
  return TDT_OK;
}

}  // extern "C"
