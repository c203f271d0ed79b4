// First-hit guide images and the edge-stopping denoiser (include/tdt_rt.h, tdt_dispatch_guide / tdt_image_denoise).
//
// Guide: one lane per texel traces the primary ray of its pixel through query_first_hit (query_device.hpp: the traversal the
// query unit runs) and stores four words of the record — the key (kind, material, plane) that says "same surface" exactly,
// and the depth.  Voxel faces are axis-aligned, so the key needs no tolerance.
//
// Filter: an a-trous wavelet filter, B3 kernel, whose only edge-stopping function is equality of the key.  The tap order and the
// operation order are fixed per pixel (tdt_rt.h) in the one filter body of denoise_device.hpp, which the kernels below instantiate
// key-only, so they all give the same bits: for steps 1 and 2 a block stages its 32x8 tile and the 2*step halo in LDS — colour and
// key, 32 B per texel, read once from memory instead of 25 times — and for steps >= 4, where the taps of neighbouring lanes no
// longer overlap, each lane gathers its 25 taps directly.  This file also owns the scratch sequence the passes of both filters run
// through; the host frame of an image call (handles, grid, pass loop) is tdt_internal.hpp's.
#include <new>
#include <string>

#include "tdt_internal.hpp"
#include "query_device.hpp"
#include "denoise_device.hpp"

namespace tdt {

__global__ __launch_bounds__(256) void guide_kernel(const TraceParams P, int sample, int all_materials, uint4 *__restrict__ guide, int gw, int gh,
                                                    uint32_t tiles_x) {
  __shared__ uint16_t s_escape[1];                   // fetch_node's LDS table of zero entries (query_node_source)
  if (threadIdx.x == 0) s_escape[0] = (uint16_t)kPackedEscape;
  __syncthreads();
  int x, y;
  ray_tile_pixel(tiles_x, x, y);                     // (a 16x16 tile of texels: neighbouring rays walk the same cells)
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

// ---- the filter: denoise_device.hpp's one body, key-only, over the staged tile or a gather ----
// steps 1 and 2: the tile and its halo of 2 * S texels through LDS, colour + key
template <int S>
__global__ __launch_bounds__(256) void denoise_tile_kernel(const float4 *__restrict__ in, const uint4 *__restrict__ guide, float4 *__restrict__ out,
                                                           int w, int h, uint32_t tiles_x) {
  constexpr int N = (kTileW + 4 * S) * (kTileH + 4 * S);
  __shared__ float4 s_col[N];
  __shared__ uint4 s_key[N];
  filter_tile<S, false>(in, guide, out, 0.f, 0.f, w, h, tiles_x, s_col, s_key, nullptr);
}

// steps >= 4: every lane gathers its own taps
__global__ __launch_bounds__(256) void denoise_gather_kernel(const float4 *__restrict__ in, const uint4 *__restrict__ guide, float4 *__restrict__ out,
                                                             int w, int h, int step, uint32_t tiles_x) {
  filter_gather<false>(in, guide, out, 0.f, 0.f, w, h, step, tiles_x);
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
  const tdt_compute *cam = tdt::camera_program(c);
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
  dim3 grid;
  uint32_t tiles_x;
  if (int rc = tdt::image_grid(ctx, g->w, g->h, tdt::kRayTile, tdt::kRayTile, "guide image too large", grid, tiles_x)) return rc;
  TDT_HIP(ctx, hipSetDevice(m->device));
  hipLaunchKernelGGL(tdt::guide_kernel, grid, dim3(256), 0, m->stream, P, sample, all ? 1 : 0, (uint4 *)g->dev, g->w, g->h, tiles_x);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_image_denoise(tdt_image *img, const tdt_image *guide, int passes, uint32_t flags) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  if (!guide) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null guide image");
  const tdt_image *handles[2] = {img, guide}, *im[2];
  if (int rc = tdt::images_of_context(ctx, handles, 2, "guide image belongs to another context")) return rc;
  if (int rc = tdt::images_fit(ctx, handles, 2, 2, im, "image and guide differ in size", "the guide is the image itself (or shares its memory)")) return rc;
  if (passes < 0 || passes > tdt::kMaxPasses) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "passes must be 0..8");
  if (flags != 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "flags must be 0");
  if (passes == 0) return TDT_OK;
  const tdt_image *a = im[0];
  const uint4 *G = (const uint4 *)im[1]->dev;
  return tdt::run_passes(ctx, a, passes, tdt::kTileW, tdt::kTileH,
                         [&](auto tile, int step, dim3 grid, hipStream_t st, const float *from, float *to, uint32_t tiles_x) {
    constexpr int S = decltype(tile)::value;
    const float4 *src = (const float4 *)from;
    float4 *dst = (float4 *)to;
    if constexpr (S == 0) hipLaunchKernelGGL(tdt::denoise_gather_kernel, grid, dim3(256), 0, st, src, G, dst, a->w, a->h, step, tiles_x);
    else hipLaunchKernelGGL(tdt::denoise_tile_kernel<S>, grid, dim3(256), 0, st, src, G, dst, a->w, a->h, tiles_x);
  });
}

}  // extern "C"
