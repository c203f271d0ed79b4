// Screen-space selection (include/tdt_rt.h, tdt_dispatch_voxel_ids / tdt_image_overlay / tdt_image_extract_voxels): where the
// Morton-sorted voxel lists of the editing units meet the images of the image units.
//
// Ids: one lane per texel traces the primary ray of its pixel through query_first_hit (query_device.hpp), as guide_kernel does,
// and turns the record into the grid voxel a click on that pixel would act on: pick_cell's arithmetic (host_scene.cpp), in
// fp64, every operation rounded on its own.  The image depends on camera and tree only.
//
// Overlay: the host list becomes sorted unique keys through the voxel-list layer (tdt_voxlist.hip, sort_pairs_u32); a block
// then stages its 32x8 tile of the id image and a halo of edge_width texels through stage_tile (denoise_device.hpp), the binary
// search for membership running once per staged texel, and every lane looks at its window in LDS only.
//
// Extract: the (key, material + 1) pairs of a rectangle's texels in row-major order, the stable sort, the last-of-run unique (the
// builder's rule: the last texel wins) and the list's tail (list_to_host).
#include <cmath>
#include <string>
#include <vector>

#include "tdt_internal.hpp"
#include "device_scan.hpp"
#include "region_device.hpp"
#include "query_device.hpp"
#include "denoise_device.hpp"

namespace tdt {

// ---- ids ----
struct IdArgs {
  double min[3], scale;                              // OctreeFloats, widened (exact)
  double cells, half, side;                          // 2^depth, 0.5 / 2^depth, +1 (place) / -1 (remove)
};

// one axis of pick_cell: the subtraction, the divide and the add round; side * n * half and q * cells are exact
TDT_DEV bool pick_axis(const IdArgs &A, int a, float point, float normal, int &k) {
  const double q = ((double)point - A.min[a]) / A.scale + A.side * (double)normal * A.half;
  const double f = __builtin_floor(q * A.cells);
  const bool ok = f >= 0.0 && f < A.cells;           // (a NaN fails)
  k = ok ? (int)f : 0;
  return ok;
}

__global__ __launch_bounds__(256) void voxel_ids_kernel(const TraceParams P, const IdArgs A, int sample, uint4 *__restrict__ ids, int gw, int gh,
                                                        uint32_t tiles_x) {
  __shared__ uint16_t s_escape[1];                   // fetch_node's LDS table of zero entries (query_node_source)
  if (threadIdx.x == 0) s_escape[0] = (uint16_t)kPackedEscape;
  __syncthreads();
  int x, y;
  ray_tile_pixel(tiles_x, x, y);
  if (x >= gw || y >= gh) return;
  const NodeSource ns = query_node_source(P, s_escape);
  const Ray r = primary_ray(P, x, y, sample);
  const QueryRecord q = query_first_hit(P, ns, r);
  uint32_t state = 0u, key = 0u;
  if (q.status == TDT_RAY_HIT && q.fresh) {
    int kx, ky, kz;
    const bool okx = pick_axis(A, 0, q.rec.px, q.rec.nx, kx), oky = pick_axis(A, 1, q.rec.py, q.rec.ny, ky),
               okz = pick_axis(A, 2, q.rec.pz, q.rec.nz, kz);
    if (okx && oky && okz) { state = 1u; key = region_key(kx, ky, kz); }
  }
  ids[(size_t)y * (size_t)gw + (size_t)x] = make_uint4(state, key, q.material, __float_as_uint(q.t));
}

// ---- the list of an overlay: {x, y, z, m} -> key; a coordinate outside [0, 1024) -> dropped ----
__global__ __launch_bounds__(256) void overlay_list_keys_kernel(const int4 *__restrict__ vox, uint32_t n, uint32_t *__restrict__ keys,
                                                                uint32_t *__restrict__ vals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 v = vox[i];
  const bool ok = ((uint32_t)v.x | (uint32_t)v.y | (uint32_t)v.z) < 1024u;
  keys[i] = ok ? region_key(v.x, v.y, v.z) : kDroppedKey;
  vals[i] = 0u;
}

// ---- overlay ----
struct OverlayArgs {
  float fill[4], edge[4];
  int w, h;
  uint32_t tiles_x, voxel_edges;
};

// The counts live in kOverlayCountSlots groups of four words, each on a 128-byte line of its own, as tdt_upsample.hip's do; the
// line behind them holds the number of unique keys of the call's list, which the kernel reads.
constexpr uint32_t kOverlayCountSlots = 64, kOverlayCountStride = 16;   // (words of 8 bytes between two groups)
constexpr size_t kOverlayCountWords = (size_t)kOverlayCountSlots * kOverlayCountStride;
constexpr size_t kOverlayCountBytes = (kOverlayCountWords + kOverlayCountStride) * sizeof(unsigned long long);

enum : uint32_t { STAGED_MEMBER = 1u, STAGED_INSIDE = 2u };

// EW = edge_width: a block's 32x8 tile and a halo of EW texels.  s_key[t] = (state, key, material, inside) of texel t, s_in[t] =
// STAGED_INSIDE for a texel of the image, with STAGED_MEMBER where its key is in the list.
template <int EW>
__global__ __launch_bounds__(256) void overlay_kernel(const OverlayArgs A, const uint4 *__restrict__ ids, float4 *__restrict__ img,
                                                      const uint32_t *__restrict__ keys, const uint32_t *__restrict__ n_keys,
                                                      unsigned long long *__restrict__ counts) {
  constexpr int TW = kTileW + 2 * EW, N = TW * (kTileH + 2 * EW);
  __shared__ uint32_t s_count[4];
  __shared__ uint4 s_key[N];
  __shared__ uint32_t s_in[N];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0u;
  int x0, y0;
  tile_origin(A.tiles_x, x0, y0);
  const uint32_t nk = *n_keys;
  stage_tile<EW>(ids, A.w, A.h, x0, y0, s_key,
                 [&](size_t p) {
                   const uint4 t = ids[p];
                   uint32_t f = STAGED_INSIDE;
                   if (t.x == 1u) {
                     const uint32_t lo = lower_bound_u32(keys, nk, t.y);
                     if (lo < nk && keys[lo] == t.y) f |= STAGED_MEMBER;
                   }
                   return f;
                 },
                 [&](int t, uint32_t f) { s_in[t] = f; });
  const int lx = (int)(threadIdx.x % kTileW), ly = (int)(threadIdx.x / kTileW);
  const int x = x0 + lx, y = y0 + ly;
  const bool inside = x < A.w && y < A.h;
  bool state1 = false, member = false, edge = false;
  if (inside) {
    const int centre = (ly + EW) * TW + lx + EW;
    const uint4 ck = s_key[centre];
    state1 = ck.x == 1u;
    member = (s_in[centre] & STAGED_MEMBER) != 0u;
    if (member) {
#pragma unroll
      for (int j = -EW; j <= EW; j++)
#pragma unroll
        for (int i = -EW; i <= EW; i++) {
          if (i == 0 && j == 0) continue;
          const int t = centre + j * TW + i;
          const uint32_t f = s_in[t];
          if (!(f & STAGED_INSIDE)) continue;
          if (!(f & STAGED_MEMBER) || (A.voxel_edges && s_key[t].y != ck.y)) edge = true;   // (a member has state 1)
        }
      const size_t p = (size_t)y * (size_t)A.w + (size_t)x;
      const float4 in = img[p];
      const float cr = edge ? A.edge[0] : A.fill[0], cg = edge ? A.edge[1] : A.fill[1], cb = edge ? A.edge[2] : A.fill[2];
      const float a = edge ? A.edge[3] : A.fill[3];
      const float keep = 1.0f - a;
      img[p] = make_float4((in.x * keep) + (cr * a), (in.y * keep) + (cg * a), (in.z * keep) + (cb * a), in.w);
    }
  }
  // the block's counts: one LDS add per wave and counter, then one global add per counter into the block's group
  const unsigned long long m0 = __ballot(inside), m1 = __ballot(state1), m2 = __ballot(member), m3 = __ballot(edge);
  if ((threadIdx.x & 63u) == 0u) {
    if (m0) atomicAdd(&s_count[0], (uint32_t)__popcll(m0));
    if (m1) atomicAdd(&s_count[1], (uint32_t)__popcll(m1));
    if (m2) atomicAdd(&s_count[2], (uint32_t)__popcll(m2));
    if (m3) atomicAdd(&s_count[3], (uint32_t)__popcll(m3));
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_count[threadIdx.x])
    atomicAdd(&counts[(blockIdx.x & (kOverlayCountSlots - 1u)) * kOverlayCountStride + threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

// ---- extract: texel i (row-major) of the rw-wide rectangle at (rx, ry) -> (key, material + 1); not selected -> dropped ----
__global__ __launch_bounds__(256) void rect_pairs_kernel(const uint4 *__restrict__ ids, int w, int rx, int ry, uint32_t rw, uint32_t n,
                                                         uint32_t *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t *__restrict__ bad) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t row = i / rw, col = i - row * rw;
  const uint4 t = ids[(size_t)(ry + (int)row) * (size_t)w + (size_t)(rx + (int)col)];
  const bool sel = t.x == 1u;
  keys[i] = sel ? t.y : kDroppedKey;
  vals[i] = t.z + 1u;
  if (sel && t.z >= 254u) *bad = 1u;
}

namespace {

const char *kNoMemory = "out of device memory in the selection";

template <int EW>
void launch_overlay(dim3 grid, hipStream_t st, const OverlayArgs &A, const uint4 *ids, float4 *img, const uint32_t *keys, const uint32_t *n_keys,
                    unsigned long long *counts) {
  hipLaunchKernelGGL(overlay_kernel<EW>, grid, dim3(256), 0, st, A, ids, img, keys, n_keys, counts);
}

// grow-only device memory of the overlay's list on the member context
int select_scratch(tdt_ctx *front, tdt_ctx *m, size_t bytes, char **out) {
  if (m->select_bytes < bytes) {
    TDT_HIP(front, hipStreamSynchronize(m->stream));            // (an overlay queued earlier may still read the old one)
    if (m->select) (void)hipFree(m->select);
    m->select = nullptr; m->select_bytes = 0;
    const hipError_t e = hipMalloc(&m->select, bytes);
    if (e != hipSuccess) { m->select = nullptr; return hip_fail(front, e, "hipMalloc (overlay list)"); }
    m->select_bytes = bytes;
  }
  *out = (char *)m->select;
  return TDT_OK;
}

// n pairs behind their stable sort into the unique (uk, uv) and *count, all in device memory: last-of-run flags, their scan, the
// gather.  k / v: the sorted pair, (uk, uv): the pair the sort left free.
int unique_sorted(tdt_ctx *front, hipStream_t st, const uint32_t *k, const uint32_t *v, uint32_t n, uint32_t *flag, uint32_t *fscr, uint32_t *uk,
                  uint32_t *uv, uint32_t *count) {
  voxlist_last_flags(st, k, n, flag);
  TDT_HIP(front, exclusive_scan_u32(st, flag, flag, n + 1u, fscr));
  voxlist_unique(st, k, v, n, flag, uk, uv, count);
  TDT_HIP(front, hipGetLastError());
  return TDT_OK;
}

}  // namespace

void select_scratch_destroy(tdt_ctx *ctx) {
  if (ctx->select) (void)hipFree(ctx->select);
  ctx->select = nullptr; ctx->select_bytes = 0;
  if (ctx->overlay_counts) (void)hipFree(ctx->overlay_counts);
  ctx->overlay_counts = nullptr;
}

}  // namespace tdt

extern "C" {

int tdt_dispatch_voxel_ids(tdt_compute *c, tdt_image *ids, int place, int sample) {
  if (!c) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = c->ctx;
  if (!ids) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null id image");
  if (c->kind != TDT_PROGRAM_RAYTRACER) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "voxel ids need a raytracer program (its camera)");
  if (ids->ctx != ctx) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "id image belongs to another context");
  if (sample < 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "negative sample index");
  if (place != 0 && place != 1) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "place must be 1 (the empty cell in front of the face) or 0 (the voxel behind it)");
  if (c->part_rank != 0 || c->part_world != 1)
    return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "voxel ids are an image, not a tile buffer: the program's partition must be (0, 1)");
  const tdt_compute *cam = tdt::camera_program(c);
  tdt_ctx *m = cam->ctx;
  TraceParams P;
  if (int rc = tdt::query_params(ctx, m, P)) return rc;
  if (P.max_depth < 1 || P.max_depth > 10) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "octree max_depth outside [1, 10]: the voxel's key must fit 30 bits");
  if (!(P.scale > 0.0f) || !std::isfinite(P.scale)) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "octree scale not positive and finite");
  tdt::query_camera(cam, P);
  tdt::IdArgs A;
  A.min[0] = (double)P.min_x; A.min[1] = (double)P.min_y; A.min[2] = (double)P.min_z; A.scale = (double)P.scale;
  A.cells = std::ldexp(1.0, P.max_depth); A.half = 0.5 / A.cells; A.side = place ? 1.0 : -1.0;
  const tdt_image *g = tdt::device_image(ids);
  dim3 grid;
  uint32_t tiles_x;
  if (int rc = tdt::image_grid(ctx, g->w, g->h, tdt::kRayTile, tdt::kRayTile, "id image too large", grid, tiles_x)) return rc;
  TDT_HIP(ctx, hipSetDevice(m->device));
  hipLaunchKernelGGL(tdt::voxel_ids_kernel, grid, dim3(256), 0, m->stream, P, A, sample, (uint4 *)g->dev, g->w, g->h, tiles_x);
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_image_overlay(tdt_image *img, const tdt_image *ids, const int32_t *voxels_xyzm, size_t n, const tdt_overlay *style) {
  if (!img) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = img->ctx;
  if (!ids || !style) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null id image or style");
  const tdt_image *handles[2] = {img, ids}, *im[2];
  if (int rc = tdt::images_of_context(ctx, handles, 2, "id image belongs to another context")) return rc;
  if (n && !voxels_xyzm) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null voxel list");
  if (style->edge_width < 0 || style->edge_width > 4) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "edge_width must be 0..4");
  if (style->flags & ~(uint32_t)TDT_OVERLAY_VOXEL_EDGES) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "unknown overlay flags");
  if (n > tdt::kVoxelListCap) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the list holds " + std::to_string(n) + " voxels (more than 2^26)");
  if (int rc = tdt::images_fit(ctx, handles, 2, 2, im, "image and id image differ in size", "the id image is the image itself (or shares its memory)"))
    return rc;
  tdt::OverlayArgs A;
  for (int i = 0; i < 4; i++) { A.fill[i] = style->fill[i]; A.edge[i] = style->edge[i]; }
  A.w = im[0]->w; A.h = im[0]->h;
  A.voxel_edges = (style->flags & TDT_OVERLAY_VOXEL_EDGES) ? 1u : 0u;
  dim3 grid;
  if (int rc = tdt::image_grid(ctx, A.w, A.h, tdt::kTileW, tdt::kTileH, "image too large", grid, A.tiles_x)) return rc;
  tdt_ctx *m = tdt::first_member(ctx);
  hipStream_t st = m->stream;
  TDT_HIP(ctx, hipSetDevice(m->device));
  // ---- the list: uploaded before the call returns, then keys, sort and unique, queued ----
  const uint32_t nl = (uint32_t)n;
  const uint32_t *keys = nullptr;
  uint32_t *k = nullptr, *v = nullptr, *uk = nullptr, *uv = nullptr, *flag = nullptr, *fscr = nullptr;
  if (nl) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_vox = up((size_t)nl * sizeof(int4)), b_n = up((size_t)nl * 4), b_hist = up(tdt::sort_hist_words(nl) * 4),
                 b_hscr = up(tdt::sort_scratch_words(nl) * 4), b_flag = up(((size_t)nl + 1) * 4), b_fscr = up(tdt::scan_scratch_words((size_t)nl + 1) * 4);
    char *base = nullptr;
    if (int rc = tdt::select_scratch(ctx, m, b_vox + 4 * b_n + b_hist + b_hscr + b_flag + b_fscr, &base)) return rc;
    int4 *vox = (int4 *)base; base += b_vox;
    uint32_t *k0 = (uint32_t *)base, *v0 = (uint32_t *)(base + b_n), *k1 = (uint32_t *)(base + 2 * b_n), *v1 = (uint32_t *)(base + 3 * b_n);
    base += 4 * b_n;
    uint32_t *hist = (uint32_t *)base, *hscr = (uint32_t *)(base + b_hist);
    flag = (uint32_t *)(base + b_hist + b_hscr); fscr = (uint32_t *)(base + b_hist + b_hscr + b_flag);
    TDT_HIP(ctx, hipMemcpyAsync(vox, voxels_xyzm, (size_t)nl * sizeof(int4), hipMemcpyHostToDevice, st));
    TDT_HIP(ctx, hipStreamSynchronize(st));                     // (the host array may be freed on return)
    hipLaunchKernelGGL(tdt::overlay_list_keys_kernel, dim3(tdt::blocks_of(nl)), dim3(256), 0, st, (const int4 *)vox, nl, k0, v0);
    k = k0; v = v0;
    TDT_HIP(ctx, tdt::sort_pairs_u32(st, k, v, k1, v1, nl, hist, hscr));
    uk = k == k0 ? k1 : k0; uv = v == v0 ? v1 : v0;
    keys = uk;
  }
  if (!m->overlay_counts) {
    const hipError_t e = hipMalloc((void **)&m->overlay_counts, tdt::kOverlayCountBytes);
    if (e != hipSuccess) { m->overlay_counts = nullptr; return tdt::hip_fail(ctx, e, "hipMalloc (overlay counts)"); }
  }
  TDT_HIP(ctx, hipMemsetAsync(m->overlay_counts, 0, tdt::kOverlayCountBytes, st));
  uint32_t *n_keys = (uint32_t *)(m->overlay_counts + tdt::kOverlayCountWords);
  if (nl)
    if (int rc = tdt::unique_sorted(ctx, st, k, v, nl, flag, fscr, uk, uv, n_keys)) return rc;
  const uint4 *I = (const uint4 *)im[1]->dev;
  float4 *D = (float4 *)im[0]->dev;
  switch (style->edge_width) {
    case 0: tdt::launch_overlay<0>(grid, st, A, I, D, keys, n_keys, m->overlay_counts); break;
    case 1: tdt::launch_overlay<1>(grid, st, A, I, D, keys, n_keys, m->overlay_counts); break;
    case 2: tdt::launch_overlay<2>(grid, st, A, I, D, keys, n_keys, m->overlay_counts); break;
    case 3: tdt::launch_overlay<3>(grid, st, A, I, D, keys, n_keys, m->overlay_counts); break;
    default: tdt::launch_overlay<4>(grid, st, A, I, D, keys, n_keys, m->overlay_counts); break;
  }
  TDT_HIP(ctx, hipGetLastError());
  return TDT_OK;
}

int tdt_debug_overlay_counts(tdt_ctx *ctx, uint64_t out[4]) {
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null counts");
  tdt_ctx *m = tdt::first_member(ctx);
  std::vector<unsigned long long> host(tdt::kOverlayCountWords, 0ull);
  TDT_HIP(ctx, hipSetDevice(m->device));
  if (m->overlay_counts)
    TDT_HIP(ctx, hipMemcpyAsync(host.data(), m->overlay_counts, tdt::kOverlayCountWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
  TDT_HIP(ctx, hipStreamSynchronize(m->stream));
  for (int i = 0; i < 4; i++) {
    out[i] = 0;
    for (uint32_t s = 0; s < tdt::kOverlayCountSlots; s++) out[i] += host[(size_t)s * tdt::kOverlayCountStride + i];
  }
  return TDT_OK;
}

int tdt_image_extract_voxels(const tdt_image *ids, const int32_t rect[4], int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  if (!ids) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = ids->ctx;
  if (!n_voxels) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels");
  *n_voxels = 0;
  const tdt_image *g = tdt::device_image(ids);
  long long x0 = 0, y0 = 0, x1 = g->w - 1, y1 = g->h - 1;
  if (rect) {
    x0 = rect[0] > 0 ? rect[0] : 0; y0 = rect[1] > 0 ? rect[1] : 0;
    x1 = rect[2] < x1 ? rect[2] : x1; y1 = rect[3] < y1 ? rect[3] : y1;
  }
  if (x0 > x1 || y0 > y1) return TDT_OK;
  const unsigned long long area = (unsigned long long)(x1 - x0 + 1) * (unsigned long long)(y1 - y0 + 1);
  if (area > tdt::kVoxelListCap) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "the rectangle holds " + std::to_string(area) + " texels (more than 2^26)");
  const uint32_t n = (uint32_t)area;
  tdt_ctx *m = tdt::first_member(ctx);
  hipStream_t st = m->stream;
  TDT_HIP(ctx, hipSetDevice(m->device));
  tdt::Drain drain{st};
  tdt::DeviceScratch S;
  uint32_t *k0 = S.get<uint32_t>(n), *v0 = S.get<uint32_t>(n), *k1 = S.get<uint32_t>(n), *v1 = S.get<uint32_t>(n);
  uint32_t *hist = S.get<uint32_t>(tdt::sort_hist_words(n)), *hscr = S.get<uint32_t>(tdt::sort_scratch_words(n));
  uint32_t *flag = S.get<uint32_t>((size_t)n + 1), *fscr = S.get<uint32_t>(tdt::scan_scratch_words((size_t)n + 1));
  uint32_t *words = S.get<uint32_t>(2);                          // the unique count, the material refusal
  if (!k0 || !v0 || !k1 || !v1 || !hist || !hscr || !flag || !fscr || !words) return tdt::fail(ctx, TDT_ERR_HIP, tdt::kNoMemory);
  TDT_HIP(ctx, hipMemsetAsync(words, 0, 2 * sizeof(uint32_t), st));
  hipLaunchKernelGGL(tdt::rect_pairs_kernel, dim3(tdt::blocks_of(n)), dim3(256), 0, st, (const uint4 *)g->dev, g->w, (int)x0, (int)y0,
                     (uint32_t)(x1 - x0 + 1), n, k0, v0, words + 1);
  uint32_t *k = k0, *v = v0;
  TDT_HIP(ctx, tdt::sort_pairs_u32(st, k, v, k1, v1, n, hist, hscr));
  uint32_t *uk = k == k0 ? k1 : k0, *uv = v == v0 ? v1 : v0;
  if (int rc = tdt::unique_sorted(ctx, st, k, v, n, flag, fscr, uk, uv, words)) return rc;
  uint32_t bad = 0, count = 0;
  if (int rc = tdt::read_word(ctx, st, words + 1, &bad)) return rc;
  if (bad) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "a selected texel carries a material >= 254 (not one the builder takes)");
  if (int rc = tdt::read_word(ctx, st, words, &count)) return rc;
  *n_voxels = count;
  if (!voxels_xyzm || count == 0) return TDT_OK;
  const int4 *out = nullptr;
  if (int rc = tdt::bitvol_emit_list(ctx, st, uk, uv, count, false, S, tdt::kNoMemory, &out)) return rc;
  return tdt::list_to_host(ctx, st, out, count, sizeof(int4), "voxels", voxels_xyzm, capacity, n_voxels);
}

}  // extern "C"
