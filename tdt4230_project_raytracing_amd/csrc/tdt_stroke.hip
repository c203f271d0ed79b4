// Stroke brushes (include/tdt_rt.h tdt_voxelize_stroke / tdt_octree_edit_stroke / tdt_octree_extract_stroke): the voxels of the
// grid [0, 2^depth)^3 within `radius` of a segment of the stroke — Euclidean for the round nib (a capsule), Chebyshev for the
// cube nib (a swept box) — decided exactly in integers, each with the material of the highest-index segment that covers it.
// The stages are the mesh unit's (tdt_mesh.hip):
//
//   setup    one lane per segment: a, d = b - a, L2 = d . d, the grid-clipped voxel range of its bounding box grown by the
//            radius and the number of 8^3-voxel tiles that range touches.                                   stroke_setup_kernel
//   tiles    exclusive scan of the tile counts; one lane per (segment, tile) finds its segment by a binary search of the scan
//            and culls the tile conservatively (below); a second scan over the flags compacts the surviving pairs in
//            candidate order, which is segment order.                                 stroke_tiles_kernel, stroke_pairs_kernel
//   voxels   one wave per surviving pair walks the voxels of (tile & the segment's voxel range), 64 per step, the segment's
//            constants being wave-uniform.  It runs twice: a counting pass (per-pair counts + a 64-bit total the host checks
//            against the cap before anything is sized by it), then, after a scan of the counts, the emitting pass writes
//            (Morton key, segment) at its pair's offset — so the pairs are in segment order.              stroke_voxels_kernel
//   unique   the builder's stable radix sort keeps that order inside every run of equal keys; the last of a run is the
//            highest segment (voxlist_last_flags).  Scan of the flags, then {x, y, z, material + 1} per kept key.
//                                                                                                            stroke_emit_kernel
//
// Arithmetic bound (|coordinate| <= 2^13 = TDT_STROKE_COORD_MAX, radius <= 2^11, grid side <= 2^10):
//   d = b - a                 |d_k| <= 2^14,            L2 = d . d       <= 3 * 2^28 < 2^30
//   w = p - a                 |w_k| <= 2^13 + 2^10 - 1, |w|^2 <= 3 * 9215^2 < 2^28,  |t| = |w . d| <= 3 * 9215 * 2^14 < 2^29
//   SPHERE middle test        (|w|^2 - r^2) * L2 < 2^28 * 2^30 = 2^58,  t^2 < 2^58: two 32 x 32 -> 64-bit widening multiplies
//   BOX slab test             ends |w_k -+ r| <= 9215 + 2048 < 2^14 times |d_k| <= 2^14: every cross-product < 2^28
// so the per-voxel arithmetic is 32-bit but for those two widening multiplies of the round nib; no 64 x 64-bit multiply (which
// the compiler expands into several 32-bit multiplies and adds) runs per voxel.  L2, r^2 and d are wave-uniform.  The tile
// cull's sphere test runs once per tile with the radius grown by 7 and keeps signed 64-bit products.
#include <string>

#include "device_scan.hpp"
#include "region_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr int kStrokeTile = 8;                           // voxels per tile side
constexpr unsigned long long kStrokeCap = 1ull << 26;    // candidate tiles, and covered (segment, voxel) pairs
constexpr uint32_t kStrokeItems = 1u << 20;              // points, segments

struct StrokeSeg {             // what the per-candidate tests read
  int32_t a[3], d[3];          // first end, b - a
  int32_t L2;                  // d . d
  int32_t vlo[3], vhi[3];      // voxel range inside the grid, inclusive (vhi < vlo on some axis: none)
  int32_t pad[3];
};
static_assert(sizeof(StrokeSeg) == 64, "StrokeSeg is 64 bytes");

// tiles of the grid-clipped voxel range of a segment's bounding box grown by r; 0 when the range misses the grid
__host__ __device__ inline uint32_t stroke_tile_count(const int a[3], const int b[3], int r, int N, int vlo[3], int vhi[3]) {
  uint32_t n = 1;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int f = (a[k] < b[k] ? a[k] : b[k]) - r, l = (a[k] > b[k] ? a[k] : b[k]) + r;
    f = f < 0 ? 0 : f; l = l > N - 1 ? N - 1 : l;
    vlo[k] = f; vhi[k] = l;
    n *= l >= f ? (uint32_t)((l >> 3) - (f >> 3) + 1) : 0u;
  }
  return n;
}

// is there an s in [0, 1] with lo_k <= s d_k <= hi_k on every axis (lo_k <= hi_k)?  With the axis mirrored where d_k < 0 the
// parameter's interval on axis k is [lo_k / e_k, hi_k / e_k], e_k = |d_k|; closed intervals on a line share a point iff every
// two of them do, so: against [0, 1], lo_k <= e_k and hi_k >= 0; against each other, lo_i e_j <= hi_j e_i.  An axis with e_k = 0
// has no interval, and the first two conditions read lo_k <= 0 <= hi_k for it, which also make its cross-products hold.
__device__ __forceinline__ bool stroke_slab(const int d[3], const int lo_in[3], const int hi_in[3]) {
  int e[3], lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const bool neg = d[k] < 0;
    e[k] = neg ? -d[k] : d[k]; lo[k] = neg ? -hi_in[k] : lo_in[k]; hi[k] = neg ? -lo_in[k] : hi_in[k];
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) ok = ok && lo[k] <= e[k] && hi[k] >= 0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      if (i != j) ok = ok && lo[i] * e[j] <= hi[j] * e[i];
  return ok;
}

// |p - q|^2 <= r2 for some q of the segment, w = p - a (the header's three cases)
__device__ __forceinline__ bool stroke_capsule(const int d[3], int L2, int r2, const int w[3]) {
  const int w2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], t = w[0] * d[0] + w[1] * d[1] + w[2] * d[2];
  const int u[3] = {w[0] - d[0], w[1] - d[1], w[2] - d[2]};
  const int u2 = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];                     // |p - b|^2 <= 3 * 9215^2 as well
  const int m = w2 - r2;
  const bool mid = m <= 0 || (unsigned long long)(uint32_t)m * (uint32_t)L2 <= (unsigned long long)(uint32_t)t * (uint32_t)t;
  return t <= 0 ? m <= 0 : t >= L2 ? u2 <= r2 : mid;
}

__global__ __launch_bounds__(256) void stroke_setup_kernel(const int32_t *pts, const uint32_t *segs, const int32_t *mats, int32_t material1,
                                                          uint32_t n_seg, uint32_t last_point, int radius, int N, StrokeSeg *out, uint32_t *mat,
                                                          uint32_t *count) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s > n_seg) return;
  if (s == n_seg) { count[s] = 0; return; }                  // the scan's extra item: its slot receives the total
  // (no segment list: the polyline's s - (s + 1), or the single point's dab 0 - 0)
  const uint32_t i = segs ? segs[2 * (size_t)s] : s, j = segs ? segs[2 * (size_t)s + 1] : (s < last_point ? s + 1u : last_point);
  StrokeSeg S;
  int b[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { S.a[k] = pts[3 * (size_t)i + k]; b[k] = pts[3 * (size_t)j + k]; S.d[k] = b[k] - S.a[k]; }
  S.L2 = S.d[0] * S.d[0] + S.d[1] * S.d[1] + S.d[2] * S.d[2];
  S.pad[0] = S.pad[1] = S.pad[2] = 0;
  count[s] = stroke_tile_count(S.a, b, radius, N, S.vlo, S.vhi);
  out[s] = S;
  mat[s] = (uint32_t)(mats ? mats[s] : material1);
}

// the segment of candidate g: the last one whose first candidate is <= g (a segment without candidates shares its successor's
// first candidate, so it is never the last)
__device__ __forceinline__ uint32_t stroke_find_segment(const uint32_t *first, uint32_t n_seg, uint32_t g) {
  uint32_t lo = 0, hi = n_seg;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (first[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}

// tile (in tiles) of candidate l of segment S
__device__ __forceinline__ void stroke_tile_of(const StrokeSeg &S, uint32_t l, int tile[3]) {
  const uint32_t ey = (uint32_t)((S.vhi[1] >> 3) - (S.vlo[1] >> 3) + 1), ez = (uint32_t)((S.vhi[2] >> 3) - (S.vlo[2] >> 3) + 1);
  tile[0] = (S.vlo[0] >> 3) + (int)(l / (ey * ez));
  tile[1] = (S.vlo[1] >> 3) + (int)((l / ez) % ey);
  tile[2] = (S.vlo[2] >> 3) + (int)(l % ez);
}

// The cull.  A covered voxel p of the tile [o, o + 7]^3 has a point q of the segment with |p_k - q_k| <= r on every axis (both
// metrics), so the segment meets the box [o - r, o + 7 + r]: the slab test, exact for that box.  The round nib also has
// |p - q|_2 <= r, and p is within sqrt(3 * 4^2) < 7 of c = o + 3, so c is within r + 7 of the segment: the capsule test of c with
// the radius r + 7, in 64 bits (its |w|^2 - R^2 and t^2 times L2 pass 2^58 here, once per tile).  Neither drops a covering tile.
__global__ __launch_bounds__(256) void stroke_tiles_kernel(const StrokeSeg *segs, const uint32_t *first, uint32_t n_seg, uint32_t n_cand, int radius,
                                                          int box, uint32_t *flag) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g > n_cand) return;
  if (g == n_cand) { flag[g] = 0; return; }
  const uint32_t s = stroke_find_segment(first, n_seg, g);
  const StrokeSeg S = segs[s];
  int tile[3], lo[3], hi[3];
  stroke_tile_of(S, g - first[s], tile);
#pragma unroll
  for (int k = 0; k < 3; k++) { lo[k] = tile[k] * kStrokeTile - radius - S.a[k]; hi[k] = lo[k] + kStrokeTile - 1 + 2 * radius; }
  bool keep = stroke_slab(S.d, lo, hi);
  if (keep && !box) {
    long long w2 = 0, t = 0, u2 = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const long long w = tile[k] * kStrokeTile + 3 - S.a[k];
      w2 += w * w; t += w * S.d[k]; u2 += (w - S.d[k]) * (w - S.d[k]);
    }
    const long long R2 = (long long)(radius + 7) * (radius + 7), L2 = S.L2;
    keep = t <= 0 ? w2 <= R2 : t >= L2 ? u2 <= R2 : (w2 - R2) * L2 <= t * t;
  }
  flag[g] = keep ? 1u : 0u;
}

__global__ __launch_bounds__(256) void stroke_pairs_kernel(const StrokeSeg *segs, const uint32_t *first, uint32_t n_seg, uint32_t n_cand,
                                                          const uint32_t *excl, uint2 *pairs) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_cand || excl[g + 1u] == excl[g]) return;
  const uint32_t s = stroke_find_segment(first, n_seg, g);
  int tile[3];
  stroke_tile_of(segs[s], g - first[s], tile);
  pairs[excl[g]] = make_uint2(s, (uint32_t)tile[0] | ((uint32_t)tile[1] << 7) | ((uint32_t)tile[2] << 14));
}

// one wave per pair.  EMIT false: counts[p] = covered voxels, *total += them.  EMIT true: the pairs at offset[p].
template <bool EMIT, bool BOX>
__global__ __launch_bounds__(256) void stroke_voxels_kernel(const StrokeSeg *segs, const uint2 *pairs, uint32_t n_pairs, int radius, uint32_t *counts,
                                                           unsigned long long *total, const uint32_t *offset, uint32_t *keys, uint32_t *vals) {
  const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (p >= n_pairs) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint2 pr = pairs[p];
  const StrokeSeg &S = segs[pr.x];
  int lo[3], ext[3];                                          // first candidate, candidates per axis
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int org = (int)((pr.y >> (7 * k)) & 127u) * kStrokeTile;
    const int f = S.vlo[k] > org ? S.vlo[k] : org, l = S.vhi[k] < org + kStrokeTile - 1 ? S.vhi[k] : org + kStrokeTile - 1;
    lo[k] = f; ext[k] = l - f + 1;                            // >= 1: the tile lies in the segment's tile range
  }
  const int d[3] = {S.d[0], S.d[1], S.d[2]}, a[3] = {S.a[0], S.a[1], S.a[2]};
  const int L2 = S.L2, r2 = radius * radius;
  const uint32_t cand = (uint32_t)(ext[0] * ext[1] * ext[2]);
  const uint32_t base = EMIT ? offset[p] : 0u;
  uint32_t done = 0;
  for (uint32_t c0 = 0; c0 < cand; c0 += 64u) {
    const uint32_t c = c0 + lane;
    bool hit = false;
    int x = 0, y = 0, z = 0;
    if (c < cand) {
      x = lo[0] + (int)(c / (uint32_t)(ext[1] * ext[2]));
      y = lo[1] + (int)((c / (uint32_t)ext[2]) % (uint32_t)ext[1]);
      z = lo[2] + (int)(c % (uint32_t)ext[2]);
      const int w[3] = {x - a[0], y - a[1], z - a[2]};
      if (BOX) {
        const int wl[3] = {w[0] - radius, w[1] - radius, w[2] - radius}, wh[3] = {w[0] + radius, w[1] + radius, w[2] + radius};
        hit = stroke_slab(d, wl, wh);
      } else {
        hit = stroke_capsule(d, L2, r2, w);
      }
    }
    const unsigned long long ball = __ballot(hit);
    if (EMIT && hit) {
      const uint32_t pos = base + done + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
      keys[pos] = region_key(x, y, z); vals[pos] = pr.x;
    }
    done += (uint32_t)__popcll(ball);
  }
  if (!EMIT && lane == 0) { counts[p] = done; if (done) atomicAdd(total, (unsigned long long)done); }
}

__global__ __launch_bounds__(256) void stroke_emit_kernel(const uint32_t *keys, const uint32_t *seg, uint32_t n, const uint32_t *excl,
                                                         const uint32_t *mat, int4 *out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || excl[i + 1u] == excl[i]) return;
  out[excl[i]] = region_voxel(keys[i], (int)mat[seg[i]]);
}

namespace {

const char *kNoMemory = "out of device memory in the stroke voxelisation";

// the segments a stroke stands for: the list's, or the polyline's (one point: one dab)
uint32_t segment_count(const tdt_stroke *s) { return s->segments ? s->n_segments : s->n_points ? (s->n_points > 1u ? s->n_points - 1u : 1u) : 0u; }

void segment_ends(const tdt_stroke *s, uint32_t k, int a[3], int b[3]) {
  const uint32_t i = s->segments ? s->segments[2 * (size_t)k] : k, j = s->segments ? s->segments[2 * (size_t)k + 1] : (s->n_points > 1u ? k + 1u : k);
  for (int c = 0; c < 3; c++) { a[c] = s->points[3 * (size_t)i + c]; b[c] = s->points[3 * (size_t)j + c]; }
}

// candidate tiles of the whole stroke on a grid of side 2^depth (what stroke_setup_kernel's counts sum to)
unsigned long long tile_candidates(const tdt_stroke *s, int depth) {
  unsigned long long total = 0;
  const uint32_t ns = segment_count(s);
  for (uint32_t k = 0; k < ns; k++) {
    int a[3], b[3], vlo[3], vhi[3];
    segment_ends(s, k, a, b);
    total += stroke_tile_count(a, b, s->radius, 1 << depth, vlo, vhi);
  }
  return total;
}

// everything about a stroke that does not depend on the grid, checked on the host before anything is queued
int check_stroke(tdt_ctx *ctx, const tdt_stroke *s) {
  if (!s) return fail(ctx, TDT_ERR_INVALID_VALUE, "null stroke");
  if (s->n_points && !s->points) return fail(ctx, TDT_ERR_INVALID_VALUE, "null point array");
  if (!s->segments && s->n_segments) return fail(ctx, TDT_ERR_INVALID_VALUE, "null segment array (the polyline form takes n_segments 0)");
  if (s->n_points > kStrokeItems || s->n_segments > kStrokeItems) return fail(ctx, TDT_ERR_INVALID_VALUE, "more than 2^20 points or segments");
  if (s->n_points == 0 && s->n_segments) return fail(ctx, TDT_ERR_INVALID_VALUE, "segments without points");
  if (s->shape != TDT_SHAPE_BOX && s->shape != TDT_SHAPE_SPHERE) return fail(ctx, TDT_ERR_INVALID_VALUE, "the nib is TDT_SHAPE_SPHERE or TDT_SHAPE_BOX");
  if (s->radius < 0 || s->radius > TDT_STROKE_RADIUS_MAX) return fail(ctx, TDT_ERR_INVALID_VALUE, "radius must be 0..2048");
  if (s->pad != 0) return fail(ctx, TDT_ERR_INVALID_VALUE, "pad must be 0");
  if (!s->materials && (s->material < 0 || s->material > 253)) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be 0..253");
  const uint32_t ns = segment_count(s);
  for (uint32_t k = 0; k < ns; k++) {
    if (s->segments)
      for (int e = 0; e < 2; e++)
        if (s->segments[2 * (size_t)k + e] >= s->n_points)
          return fail(ctx, TDT_ERR_INVALID_VALUE, "segment " + std::to_string(k) + ": point index " + std::to_string(s->segments[2 * (size_t)k + e]) +
                                                      " >= " + std::to_string(s->n_points) + " points");
    if (s->materials && (s->materials[k] < 1 || s->materials[k] > 254))
      return fail(ctx, TDT_ERR_INVALID_VALUE, "segment " + std::to_string(k) + ": material + 1 must be 1..254");
  }
  for (size_t i = 0; i < 3 * (size_t)s->n_points; i++)
    if (s->points[i] > TDT_STROKE_COORD_MAX || s->points[i] < -TDT_STROKE_COORD_MAX)
      return fail(ctx, TDT_ERR_INVALID_VALUE, "point " + std::to_string(i / 3) + ": a coordinate beyond +-8192");
  return TDT_OK;
}

// the stroke's voxels {x, y, z, material + 1}, Morton-sorted and unique, in device memory of ctx (allocated in S; null when
// *n == 0).  The stroke has passed check_stroke.  Queued on ctx's stream, so ordered after the work already there; synchronises.
int stroke_voxels(tdt_ctx *front, tdt_ctx *ctx, const tdt_stroke *s, int depth, DeviceScratch &S, const int4 **out, uint32_t *n) {
  *out = nullptr; *n = 0;
  const uint32_t ns = segment_count(s);
  if (ns == 0) return TDT_OK;
  const unsigned long long cand64 = tile_candidates(s, depth);
  if (cand64 > kStrokeCap)
    return fail(front, TDT_ERR_INVALID_VALUE, "the stroke enumerates " + std::to_string(cand64) + " candidate tiles (more than 2^26)");
  if (cand64 == 0) return TDT_OK;                          // nothing of it in the grid
  const uint32_t nc = (uint32_t)cand64;
  const bool box = s->shape == TDT_SHAPE_BOX;
  hipStream_t st = ctx->stream;
  // ---- setup ----
  int32_t *d_pts = S.get<int32_t>(3 * (size_t)s->n_points), *d_mats = s->materials ? S.get<int32_t>(ns) : nullptr;
  uint32_t *d_idx = s->segments ? S.get<uint32_t>(2 * (size_t)ns) : nullptr, *mat = S.get<uint32_t>(ns);
  StrokeSeg *segs = S.get<StrokeSeg>(ns);
  uint32_t *first = S.get<uint32_t>((size_t)ns + 1), *scr1 = S.get<uint32_t>(scan_scratch_words((size_t)ns + 1));
  uint32_t *flag = S.get<uint32_t>((size_t)nc + 1), *scr2 = S.get<uint32_t>(scan_scratch_words((size_t)nc + 1));
  unsigned long long *d_total = S.get<unsigned long long>(1);
  if (!d_pts || (s->materials && !d_mats) || (s->segments && !d_idx) || !mat || !segs || !first || !scr1 || !flag || !scr2 || !d_total)
    return fail(front, TDT_ERR_HIP, kNoMemory);
  TDT_HIP(front, hipMemcpyAsync(d_pts, s->points, 3 * (size_t)s->n_points * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (d_idx) TDT_HIP(front, hipMemcpyAsync(d_idx, s->segments, 2 * (size_t)ns * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (d_mats) TDT_HIP(front, hipMemcpyAsync(d_mats, s->materials, (size_t)ns * sizeof(int32_t), hipMemcpyHostToDevice, st));
  TDT_HIP(front, hipMemsetAsync(d_total, 0, sizeof *d_total, st));
  hipLaunchKernelGGL(stroke_setup_kernel, dim3(blocks_of((size_t)ns + 1)), dim3(256), 0, st, (const int32_t *)d_pts, (const uint32_t *)d_idx,
                     (const int32_t *)d_mats, s->material + 1, ns, s->n_points - 1u, s->radius, 1 << depth, segs, mat, first);
  TDT_HIP(front, exclusive_scan_u32(st, first, first, ns + 1u, scr1));
  // ---- tiles ----
  hipLaunchKernelGGL(stroke_tiles_kernel, dim3(blocks_of((size_t)nc + 1)), dim3(256), 0, st, (const StrokeSeg *)segs, (const uint32_t *)first, ns, nc,
                     s->radius, box ? 1 : 0, flag);
  TDT_HIP(front, exclusive_scan_u32(st, flag, flag, nc + 1u, scr2));
  uint32_t np = 0;
  if (int rc = read_word(front, st, flag + nc, &np)) return rc;   // the surviving pairs
  if (np == 0) return TDT_OK;
  uint2 *pairs = S.get<uint2>(np);
  uint32_t *counts = S.get<uint32_t>((size_t)np + 1), *scr3 = S.get<uint32_t>(scan_scratch_words((size_t)np + 1));
  if (!pairs || !counts || !scr3) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(stroke_pairs_kernel, dim3(blocks_of(nc)), dim3(256), 0, st, (const StrokeSeg *)segs, (const uint32_t *)first, ns, nc,
                     (const uint32_t *)flag, pairs);
  // ---- voxels: count, then emit ----
  const unsigned waves = (np + 3u) / 4u;
  TDT_HIP(front, hipMemsetAsync(counts + np, 0, sizeof(uint32_t), st));
  auto voxels = [&](auto emit, uint32_t *cnt, unsigned long long *tot, const uint32_t *off, uint32_t *k, uint32_t *v) {
    constexpr bool E = decltype(emit)::value;
    if (box) hipLaunchKernelGGL((stroke_voxels_kernel<E, true>), dim3(waves), dim3(256), 0, st, (const StrokeSeg *)segs, (const uint2 *)pairs, np,
                                s->radius, cnt, tot, off, k, v);
    else hipLaunchKernelGGL((stroke_voxels_kernel<E, false>), dim3(waves), dim3(256), 0, st, (const StrokeSeg *)segs, (const uint2 *)pairs, np,
                            s->radius, cnt, tot, off, k, v);
  };
  voxels(std::false_type{}, counts, d_total, nullptr, nullptr, nullptr);
  TDT_HIP(front, hipGetLastError());
  unsigned long long covered = 0;
  TDT_HIP(front, hipMemcpyAsync(&covered, d_total, sizeof covered, hipMemcpyDeviceToHost, st));
  TDT_HIP(front, hipStreamSynchronize(st));                // the covered (segment, voxel) pairs
  if (covered > kStrokeCap)
    return fail(front, TDT_ERR_INVALID_VALUE, "the stroke covers " + std::to_string(covered) + " (segment, voxel) pairs (more than 2^26)");
  if (covered == 0) return TDT_OK;                         // (a surviving tile may hold no covered voxel)
  const uint32_t nk = (uint32_t)covered;
  uint32_t *k0 = S.get<uint32_t>(nk), *v0 = S.get<uint32_t>(nk), *k1 = S.get<uint32_t>(nk), *v1 = S.get<uint32_t>(nk);
  uint32_t *hist = S.get<uint32_t>(sort_hist_words(nk)), *hscr = S.get<uint32_t>(sort_scratch_words(nk));
  uint32_t *last = S.get<uint32_t>((size_t)nk + 1), *scr4 = S.get<uint32_t>(scan_scratch_words((size_t)nk + 1));
  int4 *vox = S.get<int4>(nk);
  if (!k0 || !v0 || !k1 || !v1 || !hist || !hscr || !last || !scr4 || !vox) return fail(front, TDT_ERR_HIP, kNoMemory);
  TDT_HIP(front, exclusive_scan_u32(st, counts, counts, np + 1u, scr3));
  voxels(std::true_type{}, nullptr, nullptr, counts, k0, v0);
  // ---- sort, last of each run, materials ----
  uint32_t *k = k0, *v = v0;
  TDT_HIP(front, sort_pairs_u32(st, k, v, k1, v1, nk, hist, hscr));
  voxlist_last_flags(st, k, nk, last);
  TDT_HIP(front, exclusive_scan_u32(st, last, last, nk + 1u, scr4));
  hipLaunchKernelGGL(stroke_emit_kernel, dim3(blocks_of(nk)), dim3(256), 0, st, (const uint32_t *)k, (const uint32_t *)v, nk, (const uint32_t *)last,
                     (const uint32_t *)mat, vox);
  TDT_HIP(front, hipGetLastError());
  uint32_t nu = 0;
  if (int rc = read_word(front, st, last + nk, &nu)) return rc;   // the voxel count
  *out = vox; *n = nu;
  return TDT_OK;
}

struct StrokeSource final : VoxelSource {
  const tdt_stroke *stroke;
  explicit StrokeSource(const tdt_stroke *s) : stroke(s) {}
  int run(tdt_ctx *front, tdt_ctx *ctx, int depth, DeviceScratch &S, const int4 **vox, uint32_t *n) override {
    return stroke_voxels(front, ctx, stroke, depth, S, vox, n);
  }
};

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_voxelize_stroke(tdt_ctx *ctx, const tdt_stroke *stroke, int depth, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  if (depth < 1 || depth > 10) return fail(ctx, TDT_ERR_INVALID_VALUE, "depth must be 1..10");
  if (int rc = check_stroke(ctx, stroke)) return rc;
  StrokeSource src(stroke);
  return region_extract_source(ctx, src, depth, voxels_xyzm, capacity, n_voxels);
}

int tdt_octree_edit_stroke(tdt_ctx *ctx, int op, const tdt_stroke *stroke, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (op < TDT_REGION_SET || op > TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  if (int rc = check_stroke(ctx, stroke)) return rc;
  StrokeSource src(stroke);
  return region_edit_source(ctx, op, src, n_cells);
}

int tdt_octree_extract_stroke(tdt_ctx *ctx, const tdt_stroke *stroke, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  if (int rc = check_stroke(ctx, stroke)) return rc;
  StrokeSource src(stroke);
  return region_intersect_source(ctx, src, voxels_xyzm, capacity, n_voxels);
}

}  // extern "C"
