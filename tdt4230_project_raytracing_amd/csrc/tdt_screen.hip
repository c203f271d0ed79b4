// Through-selection (include/tdt_rt.h, tdt_octree_extract_screen / tdt_octree_edit_screen / tdt_debug_screen_counts): the marquee,
// lasso and mask that pick every voxel behind a screen shape, not only the visible ones.  It is a test per voxel, not per pixel:
//
//   V        the walk of the bound tree, expanded to its Morton-sorted voxel list (tree_voxels), as every list-based unit has it
//   select   one lane per voxel of V: the voxel's centre (or, TDT_SCREEN_WINDOW, its eight corners) goes through Q, the projection
//            of temporal reprojection (view_rows on the host, view_project on the device: reproject_device.hpp), and the pixel it
//            lands in is tested against the shape: a rectangle, a polygon by the even-odd rule in exact integers, or a mask image.
//            Then the material and distance filters.  The kernel writes label[i] in {0, 1} with the table selected = {0, 1}: the
//            VoxelSelect contract of tdt_region.hip.
//   apply    region_extract_selected / region_edit_selected: the V-only path of region edits, so the list never leaves the
//            device for an edit and every replica is edited.
//
// The polygon's doubled vertices are staged once per block in LDS and read wave-uniformly in the edge loop; a lane outside the
// polygon's pixel bounding box is no candidate, and a wave without candidates skips the loop.  The edge test multiplies two
// 32-bit differences into 64 bits (|P - A| < 2^26, |B - A| < 2^23); a 32-bit path for small coordinates is not built.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "tdt_internal.hpp"
#include "trace_params.h"
#include "reproject_device.hpp"

namespace tdt {

constexpr int kMaxScreenSide = 1 << 24;              // (float)side is exact up to here: fx < (float)image_width then bounds (int)fx
constexpr int kMaxScreenCoord = 1 << 20;             // |polygon coordinate|

struct ScreenArgs {
  ViewRows view;
  float fw, fh;                                      // (float)image_width, (float)image_height
  float min[3], scale, half;                         // OctreeFloats; half = 2^-(depth + 1)
  int shape;
  int rect[4];                                       // RECT: x0, y0, x1, y1; POLYGON: its pixel bounding box, x0 <= px < x1, y0 <= py < y1
  uint32_t n_vertices;
  int mask_w;
  int material;                                      // -1: any; else the voxel's w - 1
  float min_d2, max_d2;
};

// one tested point of a voxel, given on the doubled grid (centre: 2k + 1, corner: 2(k + c)): u = k2 * 2^-(depth + 1) is exact, the
// world point two rounded operations, then Q.  d = the world point minus the origin, on = in front and on screen.
struct ScreenPoint { float dx, dy, dz; int px, py; bool on; };
TDT_DEV ScreenPoint screen_point(const ScreenArgs &A, int x2, int y2, int z2) {
  ScreenPoint p;
  const float wx = (((float)x2 * A.half) * A.scale) + A.min[0];
  const float wy = (((float)y2 * A.half) * A.scale) + A.min[1];
  const float wz = (((float)z2 * A.half) * A.scale) + A.min[2];
  p.dx = wx - A.view.org[0]; p.dy = wy - A.view.org[1]; p.dz = wz - A.view.org[2];
  float nw, fx, fy;
  view_project(A.view, p.dx, p.dy, p.dz, nw, fx, fy);
  p.on = nw > 0.f && fx >= 0.f && fx < A.fw && fy >= 0.f && fy < A.fh;     // (a NaN fails)
  p.px = p.on ? (int)fx : 0; p.py = p.on ? (int)fy : 0;
  return p;
}

// the shape test of pixel (px, py) for the lanes with cand set; s_poly: the block's doubled vertices.  Wave-uniform control flow.
TDT_DEV bool screen_inside(const ScreenArgs &A, const int2 *s_poly, const float4 *__restrict__ mask, bool cand, int px, int py) {
  if (A.shape == TDT_SCREEN_RECT) return cand && px >= A.rect[0] && px <= A.rect[2] && py >= A.rect[1] && py <= A.rect[3];
  if (A.shape == TDT_SCREEN_MASK) {
    float m = 0.f;
    if (cand) m = mask[(size_t)py * (size_t)A.mask_w + (size_t)px].x;
    return m > 0.0f;                                 // (NaN and -0 are outside)
  }
  // a pixel inside has a crossing at or left of it and one strictly right of it, on a scan line between two vertex rows
  cand = cand && px >= A.rect[0] && px < A.rect[2] && py >= A.rect[1] && py < A.rect[3];
  if (__ballot(cand) == 0ull) return false;
  const int Px = 2 * px + 1, Py = 2 * py + 1;
  uint32_t odd = 0u;
  int2 a = s_poly[A.n_vertices - 1u];
  for (uint32_t j = 0; j < A.n_vertices; j++) {
    const int2 b = s_poly[j];
    const int ex = b.x - a.x, ey = b.y - a.y;         // (wave-uniform)
    if ((a.y > Py) != (b.y > Py)) {
      const long long s = (long long)(Px - a.x) * (long long)ey - (long long)ex * (long long)(Py - a.y);
      if (ey > 0 ? s < 0 : s > 0) odd ^= 1u;
    }
    a = b;
  }
  return cand && odd != 0u;
}

// label[i] = voxel i of V is selected; counts: [0] voxels, [1] all tested points in front and on screen, [2] of those inside the
// shape, [3] selected
template <bool WINDOW>
__global__ __launch_bounds__(256) void screen_select_kernel(const ScreenArgs A, const int4 *__restrict__ v, uint32_t n, const int2 *__restrict__ poly,
                                                            const float4 *__restrict__ mask, uint32_t *__restrict__ label,
                                                            unsigned long long *__restrict__ counts) {
  __shared__ int2 s_poly[TDT_SCREEN_MAX_VERTICES];
  __shared__ uint32_t s_count[4];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0u;
  if (A.shape == TDT_SCREEN_POLYGON && threadIdx.x < A.n_vertices) {
    const int2 q = poly[threadIdx.x];
    s_poly[threadIdx.x] = make_int2(2 * q.x, 2 * q.y);
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool live = i < n;
  const int4 p = live ? v[i] : make_int4(0, 0, 0, 0);
  const ScreenPoint c = screen_point(A, 2 * p.x + 1, 2 * p.y + 1, 2 * p.z + 1);
  bool on = live, in = live;
  if (WINDOW) {
    for (int k = 0; k < 8; k++) {
      const ScreenPoint q = screen_point(A, 2 * (p.x + (k >> 2)), 2 * (p.y + ((k >> 1) & 1)), 2 * (p.z + (k & 1)));
      on = on && q.on;
      in = screen_inside(A, s_poly, mask, on && in, q.px, q.py);
      if (__ballot(on) == 0ull) break;                // (no lane of the wave has anything left to count)
    }
  } else {
    on = on && c.on;
    in = screen_inside(A, s_poly, mask, on, c.px, c.py);
  }
  bool sel = in && (A.material < 0 || p.w - 1 == A.material);
  const float dd = (c.dz * c.dz + c.dy * c.dy) + c.dx * c.dx;
  sel = sel && A.min_d2 <= dd && dd <= A.max_d2;
  if (live) label[i] = sel ? 1u : 0u;
  // the block's counts: one LDS add per wave and counter, then one global add per counter
  const unsigned long long m0 = __ballot(live), m1 = __ballot(on), m2 = __ballot(in), m3 = __ballot(sel);
  if ((threadIdx.x & 63u) == 0u) {
    if (m0) atomicAdd(&s_count[0], (uint32_t)__popcll(m0));
    if (m1) atomicAdd(&s_count[1], (uint32_t)__popcll(m1));
    if (m2) atomicAdd(&s_count[2], (uint32_t)__popcll(m2));
    if (m3) atomicAdd(&s_count[3], (uint32_t)__popcll(m3));
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

namespace {

const char *kNoMemory = "out of device memory in the through-selection";

// what one call asks for, checked on the host before anything is queued (its host arrays outlive the copies queued from them:
// region edits drain the stream before they return)
struct ScreenSelection final : VoxelSelect {
  ScreenArgs A;
  bool window = false;
  std::vector<int2> polygon;
  const float4 *mask = nullptr;                       // device memory of device_ids[0]
  tdt_ctx *counted = nullptr;                         // the member whose counts the call reports
  unsigned long long counts[4] = {0, 0, 0, 0};        // written by the stream; the call reads them after it has drained

  int run(tdt_ctx *front, tdt_ctx *ctx, const int4 *v, uint32_t nv, int depth, DeviceScratch &S, const uint32_t **label_out,
          const uint32_t **selected_out) override {
    if (int rc = voxlist_within_cap(front, nv)) return rc;
    hipStream_t st = ctx->stream;
    uint32_t *label = S.get<uint32_t>(nv), *selected = S.get<uint32_t>(2);
    unsigned long long *d_counts = S.get<unsigned long long>(4);
    int2 *d_poly = polygon.empty() ? nullptr : S.get<int2>(polygon.size());
    if (!label || !selected || !d_counts || (!polygon.empty() && !d_poly)) return fail(front, TDT_ERR_HIP, kNoMemory);
    static const uint32_t kTable[2] = {0u, 1u};
    TDT_HIP(front, hipMemcpyAsync(selected, kTable, sizeof kTable, hipMemcpyHostToDevice, st));
    TDT_HIP(front, hipMemsetAsync(d_counts, 0, 4 * sizeof(unsigned long long), st));
    if (d_poly) TDT_HIP(front, hipMemcpyAsync(d_poly, polygon.data(), polygon.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    ScreenArgs K = A;
    K.half = std::ldexp(1.0f, -(depth + 1));
    if (window)
      hipLaunchKernelGGL(screen_select_kernel<true>, dim3(blocks_of(nv)), dim3(256), 0, st, K, v, nv, (const int2 *)d_poly, mask, label, d_counts);
    else
      hipLaunchKernelGGL(screen_select_kernel<false>, dim3(blocks_of(nv)), dim3(256), 0, st, K, v, nv, (const int2 *)d_poly, mask, label, d_counts);
    TDT_HIP(front, hipGetLastError());
    if (ctx == counted) TDT_HIP(front, hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, st));
    *label_out = label; *selected_out = selected;
    return TDT_OK;
  }
};

// every check of both entry points (edit: the call is an edit), in the header's order; nothing is queued
int make_screen_selection(tdt_ctx *ctx, const tdt_view *view, const tdt_screen_select *sel, const int32_t *polygon_xy, size_t n_vertices,
                          const tdt_image *mask, bool edit, ScreenSelection &out) {
  if (!view || !sel) return fail(ctx, TDT_ERR_INVALID_VALUE, "null view or tdt_screen_select pointer");
  if (sel->shape != TDT_SCREEN_RECT && sel->shape != TDT_SCREEN_POLYGON && sel->shape != TDT_SCREEN_MASK)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "shape must be a TDT_SCREEN_* value");
  if (sel->flags & ~(uint32_t)TDT_SCREEN_WINDOW) return fail(ctx, TDT_ERR_INVALID_VALUE, "unknown screen-selection flags");
  if (sel->material < -1 || sel->material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "the material filter must be -1 (any) or 0..253");
  if (!(sel->min_distance >= 0.f) || !(sel->max_distance >= 0.f) || sel->min_distance > sel->max_distance)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "the distances must be 0 <= min_distance <= max_distance (no NaN)");
  if (view->image_width < 2 || view->image_height < 2 || view->image_width > kMaxScreenSide || view->image_height > kMaxScreenSide)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "the view's image_width and image_height must be 2..2^24");
  std::memset(&out.A, 0, sizeof out.A);
  ScreenArgs &A = out.A;
  A.shape = sel->shape;
  for (int i = 0; i < 4; i++) A.rect[i] = sel->rect[i];
  if (sel->shape == TDT_SCREEN_POLYGON) {
    if (!polygon_xy) return fail(ctx, TDT_ERR_INVALID_VALUE, "null polygon");
    if (n_vertices < 3 || n_vertices > TDT_SCREEN_MAX_VERTICES) return fail(ctx, TDT_ERR_INVALID_VALUE, "a polygon has 3..256 vertices");
    out.polygon.resize(n_vertices);
    int lo[2] = {kMaxScreenCoord, kMaxScreenCoord}, hi[2] = {-kMaxScreenCoord, -kMaxScreenCoord};
    for (size_t j = 0; j < n_vertices; j++) {
      const int32_t q[2] = {polygon_xy[2 * j], polygon_xy[2 * j + 1]};
      for (int a = 0; a < 2; a++) {
        if (q[a] < -kMaxScreenCoord || q[a] > kMaxScreenCoord)
          return fail(ctx, TDT_ERR_INVALID_VALUE, "vertex " + std::to_string(j) + ": a coordinate beyond +-2^20");
        lo[a] = q[a] < lo[a] ? q[a] : lo[a]; hi[a] = q[a] > hi[a] ? q[a] : hi[a];
      }
      out.polygon[j] = make_int2(q[0], q[1]);
    }
    A.rect[0] = lo[0]; A.rect[1] = lo[1]; A.rect[2] = hi[0]; A.rect[3] = hi[1];
    A.n_vertices = (uint32_t)n_vertices;
  }
  if (sel->shape == TDT_SCREEN_MASK) {
    if (!mask) return fail(ctx, TDT_ERR_INVALID_VALUE, "null mask image");
    if (mask->ctx != ctx) return fail(ctx, TDT_ERR_INVALID_OPERATION, "the mask belongs to another context");
    if (edit && ctx->multi)
      return fail(ctx, TDT_ERR_INVALID_OPERATION, "a mask lives on device_ids[0] only: a multi-device context edits with a rectangle or a polygon");
    const tdt_image *g = device_image(mask);
    if (g->w != view->image_width || g->h != view->image_height)
      return fail(ctx, TDT_ERR_INVALID_VALUE, "the mask is not image_width x image_height of the view");
    out.mask = (const float4 *)g->dev;
    A.mask_w = g->w;
  }
  if (!view_rows(*view, A.view)) return fail(ctx, TDT_ERR_INVALID_VALUE, "the view is degenerate (determinant zero or not finite)");
  A.fw = (float)view->image_width; A.fh = (float)view->image_height;
  tdt_ctx *m = first_member(ctx);
  TraceParams P;
  if (int rc = query_params(ctx, m, P)) return rc;                 // slots 0, 6, 7
  if (P.max_depth < 1 || P.max_depth > 10) return fail(ctx, TDT_ERR_INVALID_VALUE, "octree max_depth outside [1, 10]");
  if (!(P.scale > 0.0f) || !std::isfinite(P.scale)) return fail(ctx, TDT_ERR_INVALID_VALUE, "octree scale not positive and finite");
  A.min[0] = P.min_x; A.min[1] = P.min_y; A.min[2] = P.min_z; A.scale = P.scale;
  A.material = sel->material;
  A.min_d2 = sel->min_distance * sel->min_distance; A.max_d2 = sel->max_distance * sel->max_distance;
  out.window = (sel->flags & TDT_SCREEN_WINDOW) != 0u;
  out.counted = m;
  return TDT_OK;
}

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_extract_screen(tdt_ctx *ctx, const tdt_view *view, const tdt_screen_select *sel, const int32_t *polygon_xy, size_t n_vertices,
                              const tdt_image *mask, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  ScreenSelection S;
  if (int rc = make_screen_selection(ctx, view, sel, polygon_xy, n_vertices, mask, false, S)) return rc;
  if (int rc = region_extract_selected(ctx, S, voxels_xyzm, capacity, n_voxels)) return rc;
  for (int i = 0; i < 4; i++) ctx->screen_counts[i] = S.counts[i];
  return TDT_OK;
}

int tdt_octree_edit_screen(tdt_ctx *ctx, int op, const tdt_view *view, const tdt_screen_select *sel, const int32_t *polygon_xy,
                           size_t n_vertices, const tdt_image *mask, int32_t material, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (op != TDT_REGION_PAINT && op != TDT_REGION_CLEAR)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be TDT_REGION_PAINT or TDT_REGION_CLEAR (the selection is a subset of the tree's voxels)");
  if (material < 0 || material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be 0..253");
  ScreenSelection S;
  if (int rc = make_screen_selection(ctx, view, sel, polygon_xy, n_vertices, mask, true, S)) return rc;
  if (int rc = region_edit_selected(ctx, op, material, S, n_cells)) return rc;
  for (int i = 0; i < 4; i++) ctx->screen_counts[i] = S.counts[i];
  return TDT_OK;
}

int tdt_debug_screen_counts(tdt_ctx *ctx, uint64_t out[4]) {
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null counts");
  tdt_ctx *m = tdt::first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  TDT_HIP(ctx, hipStreamSynchronize(m->stream));
  for (int i = 0; i < 4; i++) out[i] = ctx->screen_counts[i];
  return TDT_OK;
}

}  // extern "C"
