// Affine transforms of voxel selections (include/tdt_rt.h tdt_octree_transform / tdt_octree_extract_transform): move, turn,
// mirror, rotate and scale by resampling.  The map is given destination -> source, s(p) = (A (2p + 1) + t) >> 17 per axis in
// int64, so every destination voxel p looks its source voxel up and the result has no holes whatever A is:
//   T = { (p, m) : p in G & dst, s(p) in S },  S = the tree's voxels inside the mask.
//
//   source     tree_voxels, then tdt_bitvol.hip's steps over the SOURCE BOX = bbox(V) & the bounding box of the shapes & G:
//              bitvol_list_bbox, bitvol_layout, bitvol_rasterise into occupancy bits and the sorted (Morton key, material + 1)
//              pairs.  S is never formed as a list: a candidate's source voxel takes the shapes' exact integer test itself.
//   domain     on the host: dst & G & a bounding box of the preimage of the source box, from the adjugate inverse of A in long
//              double, widened by its own rounding bound plus a voxel (every candidate is tested exactly, so too wide is only
//              slower), rounded out to aligned 8 x 8 x 8 BRICKS.  A brick is a contiguous range of 512 Morton keys.
//   bricks     one lane per brick of the domain: the exact per-axis minimum and maximum of s over the brick (affine, then a
//              monotone floor: the signs of A pick the corner), kept when that box meets the source box.  Run twice around
//              exclusive_scan_u32: flags, then the kept bricks' Morton keys, compacted.                  xform_brick_kernel
//              The kept keys are sorted (tdt::sort_pairs_u32; at most 2^21 of them) so that the bricks, and the voxels inside
//              them enumerated in Morton order, come out as one Morton-sorted list with no sort of the result.
//   count,     one lane per destination voxel of a kept brick, lane = the voxel's Morton index in the brick, so a block is half
//   emit       a brick and a wave a 4 x 4 x 4 octant of it.  The brick's int64 base A (16 b + 1) + t is uniform over the block
//              (scalar 64-bit multiply-adds, once); the voxel adds A * 2d, d in 0..7, which fits an int32 under |a| <= 2^20.
//              Then the shift, the box test, the bit test, the shapes.  The wave's ballot is its count; after
//              exclusive_scan_u32 over the waves the emit pass repeats the test and writes (key, material + 1) at the wave's
//              offset + the lane's rank in the ballot, the material by bitvol_find in the sorted pairs.
//                                                                                     xform_count_kernel, xform_emit_kernel
//   list       bitvol_list_tail around the two (an item is a wave of a kept brick), without the sort.
//   synchronisations per call: the tree walk, the bounding box, the brick count, the voxel count, the end.
#include <cstring>
#include <string>
#include <vector>

#include "bitvol_device.hpp"
#include "device_scan.hpp"
#include "tdt_internal.hpp"

namespace tdt {

struct XformParams {
  BitBox B;                    // the source box and the layout of the occupancy bits over it
  long long t[3];
  int32_t a[9];
  int32_t dlo[3], dhi[3];      // dst & G & the preimage box: a destination voxel outside it is no candidate
  int32_t blo[3];              // the domain in bricks: origin and extent
  uint32_t bext[3], n_bricks;
  uint32_t fixed;              // material + 1 of every result voxel, or 0: the source voxel's
  uint32_t n_shapes;           // 0: no mask
};

// flags (excl == null): flag[i] = brick i of the domain can hold a result; keys: the kept bricks' Morton keys at excl[i]
__global__ __launch_bounds__(256) void xform_brick_kernel(const XformParams P, const uint32_t *excl, uint32_t *out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > P.n_bricks) return;
  if (i == P.n_bricks) { if (!excl) out[i] = 0; return; }   // the scan's extra item: its slot receives the total
  int b[3];
  b[0] = P.blo[0] + (int)(i % P.bext[0]);
  b[1] = P.blo[1] + (int)((i / P.bext[0]) % P.bext[1]);
  b[2] = P.blo[2] + (int)(i / (P.bext[0] * P.bext[1]));
  bool keep = true;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    long long lo = P.t[r], hi = P.t[r];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const long long a = P.a[3 * r + c], q0 = 16 * b[c] + 1, q1 = 16 * b[c] + 15;
      lo += a >= 0 ? a * q0 : a * q1;
      hi += a >= 0 ? a * q1 : a * q0;
    }
    keep = keep && (hi >> 17) >= (long long)P.B.lo[r] && (lo >> 17) <= (long long)P.B.hi[r];
  }
  if (!excl) out[i] = keep ? 1u : 0u;
  else if (keep) out[excl[i]] = region_key(b[0], b[1], b[2]);
}

// the candidate of this lane: voxel `lane` (its Morton index, 0..511) of the brick with Morton key kb.  True when its source
// voxel is in S; *sx, *sy, *sz = that voxel
__device__ __forceinline__ bool xform_hit(const XformParams &P, const uint32_t *occ, const RegionShape *shapes, uint32_t kb, uint32_t lane,
                                          int *sx, int *sy, int *sz) {
  const int b[3] = {(int)region_compact3(kb >> 2), (int)region_compact3(kb >> 1), (int)region_compact3(kb)};
  const int d[3] = {(int)region_compact3(lane >> 2), (int)region_compact3(lane >> 1), (int)region_compact3(lane)};
  bool in = true;
  long long s[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const int p = 8 * b[r] + d[r];
    in = in && p >= P.dlo[r] && p <= P.dhi[r];
    // the base is uniform over the block; the offset is at most 3 * 2^20 * 14 in magnitude
    const long long base = P.t[r] + (long long)P.a[3 * r] * (16 * b[0] + 1) + (long long)P.a[3 * r + 1] * (16 * b[1] + 1) +
                           (long long)P.a[3 * r + 2] * (16 * b[2] + 1);
    const int off = P.a[3 * r] * (2 * d[0]) + P.a[3 * r + 1] * (2 * d[1]) + P.a[3 * r + 2] * (2 * d[2]);
    s[r] = (base + off) >> 17;
    in = in && s[r] >= (long long)P.B.lo[r] && s[r] <= (long long)P.B.hi[r];
  }
  if (!in) return false;
  const int x = (int)s[0], y = (int)s[1], z = (int)s[2];
  const uint32_t row = (uint32_t)(z - P.B.lo[2]) * (uint32_t)P.B.ey + (uint32_t)(y - P.B.lo[1]);
  if (!((occ[row * (uint32_t)P.B.nw + (uint32_t)((x >> 5) - P.B.wx0)] >> (x & 31)) & 1u)) return false;
  if (P.n_shapes) {
    bool inside = false;
    for (uint32_t k = 0; k < P.n_shapes && !inside; k++) inside = region_inside(shapes[k], x, y, z);
    if (!inside) return false;
  }
  *sx = x; *sy = y; *sz = z;
  return true;
}

// grid: two blocks per kept brick; count[w] = the results of wave w (8 per brick), count[8 n_active] = 0 for the scan
__global__ __launch_bounds__(256) void xform_count_kernel(const XformParams P, const uint32_t *occ, const RegionShape *shapes, const uint32_t *bricks,
                                                         uint32_t n_active, uint32_t *count) {
  const uint32_t kb = bricks[blockIdx.x >> 1];
  const uint32_t lane = ((blockIdx.x & 1u) << 8) | threadIdx.x;
  int x, y, z;
  const unsigned long long hits = __ballot(xform_hit(P, occ, shapes, kb, lane, &x, &y, &z));
  if ((threadIdx.x & 63u) == 0) count[blockIdx.x * 4u + (threadIdx.x >> 6)] = (uint32_t)__popcll(hits);
  if (blockIdx.x == 0 && threadIdx.x == 0) count[8u * n_active] = 0;
}

__global__ __launch_bounds__(256) void xform_emit_kernel(const XformParams P, const uint32_t *occ, const RegionShape *shapes, const uint32_t *bricks,
                                                        const uint32_t *excl, const uint32_t *wkeys, const uint32_t *wvals, uint32_t n_w,
                                                        uint32_t *keys, uint32_t *vals) {
  const uint32_t kb = bricks[blockIdx.x >> 1];
  const uint32_t lane = ((blockIdx.x & 1u) << 8) | threadIdx.x;
  int x = 0, y = 0, z = 0;
  const bool hit = xform_hit(P, occ, shapes, kb, lane, &x, &y, &z);
  const unsigned long long hits = __ballot(hit);
  if (!hit) return;
  const uint32_t below = (uint32_t)__popcll(hits & ((1ull << (threadIdx.x & 63u)) - 1ull));
  const uint32_t pos = excl[blockIdx.x * 4u + (threadIdx.x >> 6)] + below;
  keys[pos] = (kb << 9) | lane;
  vals[pos] = P.fixed ? P.fixed : wvals[bitvol_find(wkeys, n_w, region_key(x, y, z))];
}

namespace {

const char *kNoMemory = "out of device memory in the transform";
constexpr long long kMaxA = 1ll << 20, kMaxT = 1ll << 40;

// what one call asks for, validated on the host before anything is queued
struct Request {
  tdt_xform x;
  long double inv[9];          // the inverse of x.a (as integers, not Q16)
  std::vector<RegionShape> shapes;
  bool masked = false;
};

int make_request(tdt_ctx *ctx, const tdt_xform *x, const tdt_region *regions, size_t n_regions, Request &R) {
  if (!x) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_xform pointer");
  for (int k = 0; k < 9; k++)
    if (x->a[k] > kMaxA || x->a[k] < -kMaxA) return fail(ctx, TDT_ERR_INVALID_VALUE, "|a| must be <= 2^20");
  for (int k = 0; k < 3; k++)
    if (x->t[k] > kMaxT || x->t[k] < -kMaxT) return fail(ctx, TDT_ERR_INVALID_VALUE, "|t| must be <= 2^40");
  if (x->material < -1 || x->material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be -1 (the source voxel's) or 0..253");
  if (x->pad[0] || x->pad[1]) return fail(ctx, TDT_ERR_INVALID_VALUE, "pad must be 0");
  const int32_t *a = x->a;
  __int128 adj[9];                                         // the adjugate: inverse = adj / det
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
      adj[3 * r + c] = (__int128)a[3 * r1 + c1] * a[3 * r2 + c2] - (__int128)a[3 * r1 + c2] * a[3 * r2 + c1];
    }
  const __int128 det = (__int128)a[0] * adj[0] + (__int128)a[1] * adj[3] + (__int128)a[2] * adj[6];
  if (det == 0) return fail(ctx, TDT_ERR_INVALID_VALUE, "the matrix is singular");
  for (int k = 0; k < 9; k++) R.inv[k] = (long double)adj[k] / (long double)det;
  R.x = *x;
  R.masked = n_regions > 0;
  return region_shapes(ctx, regions, n_regions, &R.shapes);
}

// T on one single-device context, {x, y, z, material + 1}, Morton-sorted, in device memory of ctx (allocated in S; null when
// *n == 0).  Queued on ctx's stream; synchronises.  bricks (on front): tdt_debug_xform_bricks.
int xform_list(tdt_ctx *front, tdt_ctx *ctx, const Request &R, DeviceScratch &S, const int4 **out, uint32_t *n) {
  *out = nullptr; *n = 0;
  front->xform_bricks[0] = front->xform_bricks[1] = 0;
  const tdt_xform &X = R.x;
  hipStream_t st = ctx->stream;
  int4 *v = nullptr;
  uint32_t nv = 0;
  int depth = 0;
  if (int rc = tree_voxels_capped(front, ctx, S, &v, &nv, &depth)) return rc;
  if (nv == 0) return TDT_OK;
  const long long N = 1ll << depth;
  // ---- the source box: bbox(V) & the shapes' bounding box (each shape clipped to the grid, the ones that leave it dropped;
  // tdt_geodesic.hip's host_domain unions first and clips after, which gives its domain another box: the two stay apart) ----
  int box[6];
  if (int rc = bitvol_list_bbox(front, st, v, nv, depth, S, kNoMemory, "a voxel lies outside the grid", box)) return rc;
  if (R.masked) {
    long long mlo[3] = {N, N, N}, mhi[3] = {-1, -1, -1};
    for (const RegionShape &g : R.shapes) {
      long long lo[3], hi[3];
      bool some = true;
      for (int a = 0; a < 3; a++) {
        lo[a] = g.shape == TDT_SHAPE_BOX ? g.a[a] : (long long)g.a[a] - g.b[0];
        hi[a] = g.shape == TDT_SHAPE_BOX ? g.b[a] : (long long)g.a[a] + g.b[0];
        lo[a] = lo[a] < 0 ? 0 : lo[a]; hi[a] = hi[a] > N - 1 ? N - 1 : hi[a];
        some = some && lo[a] <= hi[a];
      }
      if (!some) continue;                                 // nothing of it in the grid
      for (int a = 0; a < 3; a++) { mlo[a] = lo[a] < mlo[a] ? lo[a] : mlo[a]; mhi[a] = hi[a] > mhi[a] ? hi[a] : mhi[a]; }
    }
    for (int a = 0; a < 3; a++) {
      box[a] = mlo[a] > box[a] ? (int)mlo[a] : box[a];
      box[3 + a] = mhi[a] < box[3 + a] ? (int)mhi[a] : box[3 + a];
      if (box[a] > box[3 + a]) return TDT_OK;              // S is empty
    }
  }
  XformParams P;
  std::memset(&P, 0, sizeof P);
  bitvol_layout(box, box + 3, P.B);
  // ---- the domain: dst & G & the preimage of the source box, then whole bricks ----
  // s_r in [lo_r, hi_r]  <=>  (A q)_r in [lo_r 2^17 - t_r, (hi_r + 1) 2^17 - 1 - t_r]; q = A^-1 (A q) is bounded over that box
  // by the signs of the inverse; err bounds what long double loses (2^-50 relative per term, far above its unit roundoff)
  long double ulo[3], uhi[3];
  for (int r = 0; r < 3; r++) {
    ulo[r] = (long double)box[r] * 131072.0L - (long double)X.t[r];
    uhi[r] = (long double)(box[3 + r] + 1) * 131072.0L - 1.0L - (long double)X.t[r];
  }
  for (int c = 0; c < 3; c++) {
    long double qlo = 0, qhi = 0, err = 0;
    for (int r = 0; r < 3; r++) {
      const long double w = R.inv[3 * c + r];
      qlo += w >= 0 ? w * ulo[r] : w * uhi[r];
      qhi += w >= 0 ? w * uhi[r] : w * ulo[r];
      const long double m = (ulo[r] < 0 ? -ulo[r] : ulo[r]) > (uhi[r] < 0 ? -uhi[r] : uhi[r]) ? (ulo[r] < 0 ? -ulo[r] : ulo[r]) : (uhi[r] < 0 ? -uhi[r] : uhi[r]);
      err += (w < 0 ? -w : w) * m;
    }
    err = err * 8.8817841970012523e-16L + 2.0L;            // 2^-50, and a voxel (q is doubled)
    long double plo = (qlo - err - 1.0L) * 0.5L - 1.0L, phi = (qhi + err - 1.0L) * 0.5L + 1.0L;   // p = (q - 1) / 2
    long long lo = X.dst_lo[c] < 0 ? 0 : X.dst_lo[c], hi = X.dst_hi[c] > N - 1 ? N - 1 : X.dst_hi[c];
    if (plo > (long double)hi || phi < (long double)lo) return TDT_OK;
    if (plo > (long double)lo) lo = (long long)plo;        // truncation of a value > lo >= 0: rounds down
    if (phi < (long double)hi) hi = (long long)phi + 1 > hi ? hi : (long long)phi + 1;
    if (lo > hi) return TDT_OK;                            // an empty dst box or no preimage inside it
    P.dlo[c] = (int32_t)lo; P.dhi[c] = (int32_t)hi;
    P.blo[c] = (int32_t)(lo >> 3); P.bext[c] = (uint32_t)((hi >> 3) - (lo >> 3) + 1);
  }
  P.n_bricks = P.bext[0] * P.bext[1] * P.bext[2];          // <= 128^3
  for (int k = 0; k < 9; k++) P.a[k] = X.a[k];
  for (int k = 0; k < 3; k++) P.t[k] = X.t[k];
  P.fixed = X.material >= 0 ? (uint32_t)X.material + 1u : 0u;
  P.n_shapes = (uint32_t)R.shapes.size();
  front->xform_bricks[0] = P.n_bricks;
  // ---- the source volume ----
  uint32_t *occ = S.get<uint32_t>(P.B.n_words), *wk = S.get<uint32_t>(nv), *wv = S.get<uint32_t>(nv);
  if (!occ || !wk || !wv) return fail(front, TDT_ERR_HIP, kNoMemory);
  RegionShape *d_shapes = nullptr;
  if (int rc = upload_shapes(front, st, S, R.shapes.data(), P.n_shapes, kNoMemory, &d_shapes)) return rc;
  if (int rc = bitvol_rasterise(front, st, v, nv, P.B, occ, wk, wv)) return rc;
  // ---- bricks ----
  const size_t nb1 = (size_t)P.n_bricks + 1;
  uint32_t *flag = S.get<uint32_t>(nb1), *bscr = S.get<uint32_t>(scan_scratch_words(nb1));
  if (!flag || !bscr) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(xform_brick_kernel, dim3(blocks_of(nb1)), dim3(256), 0, st, P, (const uint32_t *)nullptr, flag);
  TDT_HIP(front, exclusive_scan_u32(st, flag, flag, (uint32_t)nb1, bscr));
  TDT_HIP(front, hipGetLastError());
  uint32_t n_active = 0;
  if (int rc = read_word(front, st, flag + P.n_bricks, &n_active)) return rc;   // the brick count
  front->xform_bricks[1] = n_active;
  if (n_active == 0) return TDT_OK;
  uint32_t *bk = S.get<uint32_t>(n_active), *bv = S.get<uint32_t>(n_active), *bk1 = S.get<uint32_t>(n_active), *bv1 = S.get<uint32_t>(n_active);
  uint32_t *hist = S.get<uint32_t>(sort_hist_words(n_active)), *hscr = S.get<uint32_t>(sort_scratch_words(n_active));
  if (!bk || !bv || !bk1 || !bv1 || !hist || !hscr) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(xform_brick_kernel, dim3(blocks_of(nb1)), dim3(256), 0, st, P, (const uint32_t *)flag, bk);
  TDT_HIP(front, hipMemsetAsync(bv, 0, (size_t)n_active * sizeof(uint32_t), st));   // the sort's values: unused
  TDT_HIP(front, sort_pairs_u32(st, bk, bv, bk1, bv1, n_active, hist, hscr));
  // ---- count, emit: 8 waves per kept brick ----
  auto count = [&](uint32_t *cnt) {
    hipLaunchKernelGGL(xform_count_kernel, dim3(n_active * 2u), dim3(256), 0, st, P, (const uint32_t *)occ, (const RegionShape *)d_shapes,
                       (const uint32_t *)bk, n_active, cnt);
  };
  auto emit = [&](const uint32_t *excl, uint32_t *keys, uint32_t *vals) {
    hipLaunchKernelGGL(xform_emit_kernel, dim3(n_active * 2u), dim3(256), 0, st, P, (const uint32_t *)occ, (const RegionShape *)d_shapes,
                       (const uint32_t *)bk, excl, (const uint32_t *)wk, (const uint32_t *)wv, nv, keys, vals);
  };
  return bitvol_list_tail(front, st, (size_t)n_active * 8, count, emit, "the result", false, nullptr, nullptr, 0u, S, kNoMemory, out, n);
}

struct XformSource final : VoxelSource {
  const Request &R;
  explicit XformSource(const Request &r) : R(r) {}
  int run(tdt_ctx *front, tdt_ctx *ctx, int, DeviceScratch &S, const int4 **vox, uint32_t *n) override { return xform_list(front, ctx, R, S, vox, n); }
};

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_transform(tdt_ctx *ctx, const tdt_xform *x, int op, const tdt_region *regions, size_t n_regions, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  Request R;
  if (int rc = make_request(ctx, x, regions, n_regions, R)) return rc;
  if (op < TDT_REGION_SET || op > TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  XformSource src(R);
  return region_edit_source(ctx, op, src, n_cells);
}

int tdt_octree_extract_transform(tdt_ctx *ctx, const tdt_xform *x, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                                 size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  Request R;
  if (int rc = make_request(ctx, x, regions, n_regions, R)) return rc;
  XformSource src(R);
  return region_extract_source(ctx, src, 0, voxels_xyzm, capacity, n_voxels);
}

int tdt_debug_xform_bricks(const tdt_ctx *ctx, uint32_t out[2]) {
  if (!ctx || !out) return TDT_ERR_INVALID_VALUE;
  out[0] = ctx->xform_bricks[0]; out[1] = ctx->xform_bricks[1];
  return TDT_OK;
}

}  // extern "C"
