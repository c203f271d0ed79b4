// Ray queries — "what is under this pixel?" (include/tdt_rt.h, tdt_raycast / tdt_raycast_device / tdt_pick_pixels).
//
// One query ray per lane runs OctreeHit (rc:397-450) as the trace kernel's general build runs it for a fresh invocation
// (zeroed Carry): root slab test, restart-from-root loop, the literal treeLookup (the float formula: right for every
// cell_count), the padded empty-cell exit and the i > 0 leaf slab test with its fall-back to the call site's old
// temporaries.  A plain gather kernel: no persistent blocks, no LDS node table, no jump tables, no bricks — node reads go
// straight to the cells buffer through a raw buffer resource whose range check is the reference's robust access.
#include <cstring>
#include <new>
#include <string>

#include "tdt_internal.hpp"
#include "trace_device.hpp"

namespace tdt {

constexpr uint32_t kQueryBlock = 256;
constexpr size_t kQueryChunk = size_t(1) << 28;      // rays per launch (32-bit lane index with room to spare)

struct QueryOut {                                    // tdt_ray_hit as four 16-byte stores
  uint4 q[4];
};

// PICK: the ray is the primary ray of pixel xy[i] and sample `sample` (rc:240-245), written to rays_out when non-null;
// otherwise it is rays[i] = {origin, direction}
template <bool PICK>
__global__ __launch_bounds__(kQueryBlock) void raycast_kernel(const TraceParams P, const float *__restrict__ rays, const int32_t *__restrict__ xy,
                                                              int sample, float *__restrict__ rays_out, QueryOut *__restrict__ hits, uint32_t n) {
  __shared__ uint16_t s_escape[1];                   // fetch_node's LDS table of zero entries: its sentinel sends every read to the buffer
  if (threadIdx.x == 0) s_escape[0] = (uint16_t)kPackedEscape;
  __syncthreads();
  const uint32_t i = blockIdx.x * kQueryBlock + threadIdx.x;
  if (i >= n) return;
  NodeSource ns;
  ns.lds = s_escape; ns.lds_nodes = 0u; ns.lds_cells = 0u;
  ns.grid = nullptr; ns.grid_ok = false; ns.grid_band = 2.0f; ns.full = nullptr; ns.grid32 = nullptr; ns.bricks = nullptr;
  ns.thr = nullptr; ns.thr_f0max = 0.0f;
  ns.cells = __builtin_amdgcn_make_buffer_rsrc((void *)P.cells, 0, (int)((P.cells_dwords >> 1) << 3), 0x00020000);

  Ray r;
  if (PICK) {
    r = primary_ray(P, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], sample);
    if (rays_out) {
      float *o = rays_out + 6 * (size_t)i;
      o[0] = r.ox; o[1] = r.oy; o[2] = r.oz; o[3] = r.dx; o[4] = r.dy; o[5] = r.dz;
    }
  } else {
    const float *a = rays + 6 * (size_t)i;
    r = {a[0], a[1], a[2], a[3], a[4], a[5]};
  }

  // OctreeHit prologue rc:399-408: the root call site (t_min = 0.0003, t_max = +inf)
  const float inf = __builtin_inff();
  float ix, iy, iz;
  q_rcp3(r.dx, r.dy, r.dz, ix, iy, iz);
  const float lx = (P.min_x + -r.ox) * ix, ly = (P.min_y + -r.oy) * iy, lz = (P.min_z + -r.oz) * iz;
  const float ux = ((P.min_x + P.scale) + -r.ox) * ix, uy = ((P.min_y + P.scale) + -r.oy) * iy, uz = ((P.min_z + P.scale) + -r.oz) * iz;
  const float mnx = hw_min(lx, ux), mny = hw_min(ly, uy), mnz = hw_min(lz, uz);
  const float mxx = hw_max(lx, ux), mxy = hw_max(ly, uy), mxz = hw_max(lz, uz);
  const float root_enter = hw_max(hw_max(hw_max(mnx, 0.0003f), mny), mnz);
  const float root_exit = hw_min(hw_min(hw_min(mxx, inf), mxy), mxz);
  const bool root_hit = root_exit >= root_enter;
  HitTmp root = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
  float root_t = 0.f, t_octree_max = inf;
  if (root_hit) {
    cube_hit_record(r, root_enter, P.min_x, P.min_y, P.min_z, P.scale, root);
    root_t = root_enter;
    t_octree_max = root_exit;
  }

  // the loop rc:410-447
  float t_stride = root_t, inv_pow_depth = 0.5f;
  int it = 0, lookups = 0, status = TDT_RAY_MISS;
  uint32_t material = 0u;
  HitTmp rec = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
  float t_rec = 0.f, cmin_x = 0.f, cmin_y = 0.f, cmin_z = 0.f, csize = 0.f;
  bool fresh = false;
  Counters cnt = {};
  for (;;) {
    if (!(it < P.max_iter && t_stride < t_octree_max)) {
      status = (t_stride < t_octree_max) ? TDT_RAY_ITER_LIMIT : TDT_RAY_MISS;
      break;
    }
    const float adv = f_max(0.0001f * (inv_pow_depth + 0.1f), 0.000001f);
    const float tt = t_stride + adv;
    const float wx = tt * r.dx + r.ox, wy = tt * r.dy + r.oy, wz = tt * r.dz + r.oz;
    const float px = (wx + -P.min_x) * P.inv_scale, py = (wy + -P.min_y) * P.inv_scale, pz = (wz + -P.min_z) * P.inv_scale;
    const float ex = f_fract(px) + -px, ey = f_fract(py) + -py, ez = f_fract(pz) + -pz;
    if ((__builtin_fabsf(ez) + __builtin_fabsf(ey)) != -__builtin_fabsf(ex)) break;    // rc:417: not in the octree -> false
    lookups++;
    const float ipd_in = inv_pow_depth;
    float gx, gy, gz; uint32_t value;
    const bool leaf = tree_lookup<false>(P, ns, px, py, pz, inv_pow_depth, gx, gy, gz, value, cnt);
    const float bx = gx * P.scale + P.min_x, by = gy * P.scale + P.min_y, bz = gz * P.scale + P.min_z;
    const float cs0 = P.scale * inv_pow_depth;
    if (leaf) {                                      // rc:421-436
      status = TDT_RAY_HIT; material = value;
      cmin_x = bx; cmin_y = by; cmin_z = bz; csize = cs0;
      if (it > 0) {
        float t_enter, t_exit;
        cube_slabs(r, ix, iy, iz, bx, by, bz, cs0, t_stride, t_octree_max, t_enter, t_exit);
        if (!(t_exit < t_enter)) { cube_hit_record(r, t_enter, bx, by, bz, cs0, rec); t_rec = t_enter; fresh = true; }
      } else {
        rec = root; t_rec = root_t; fresh = root_hit;
      }
      break;
    }
    // rc:438-446: the empty cell, padded
    float t_enter, t_exit;
    cube_slabs(r, ix, iy, iz, bx + -0.00001f, by + -0.00001f, bz + -0.00001f, cs0 + 0.00002f, t_stride, t_octree_max, t_enter, t_exit);
    const float ts_new = !(t_exit < t_enter) ? t_exit : t_octree_max;
    // a step that leaves (t_stride, inv_pow_depth) as it found them repeats itself up to max_iter (the loop body is a function of
    // those two and the ray): the shader ends at the iteration limit with every remaining iteration reaching treeLookup
    if (__float_as_uint(ts_new) == __float_as_uint(t_stride) && __float_as_uint(inv_pow_depth) == __float_as_uint(ipd_in)) {
      lookups = P.max_iter;
      status = TDT_RAY_ITER_LIMIT;
      break;
    }
    t_stride = ts_new;
    it++;
  }

  QueryOut o;
  o.q[0] = make_uint4((uint32_t)status, material, __float_as_uint(t_rec), (uint32_t)lookups);
  o.q[1] = make_uint4(__float_as_uint(rec.px), __float_as_uint(rec.py), __float_as_uint(rec.pz), __float_as_uint(rec.nx));
  o.q[2] = make_uint4(__float_as_uint(rec.ny), __float_as_uint(rec.nz), rec.ff ? 1u : 0u, fresh ? 1u : 0u);
  o.q[3] = make_uint4(__float_as_uint(cmin_x), __float_as_uint(cmin_y), __float_as_uint(cmin_z), __float_as_uint(csize));
  hits[i] = o;
}

namespace {

// the kernel arguments a query needs: slots 0, 6, 7 of the member context; errors are reported on `front`
int query_params(tdt_ctx *front, tdt_ctx *m, TraceParams &P) {
  static const int required[] = {TDT_SLOT_CELLS, TDT_SLOT_OCTREE_FLOATS, TDT_SLOT_OCTREE_INTS};
  for (int s : required)
    if (!m->ssbo[s]) return fail(front, TDT_ERR_INCOMPLETE, "no buffer bound to shader-storage slot " + std::to_string(s));
  std::memset(&P, 0, sizeof P);
  if (int rc = octree_uniforms(m, P)) return m == front ? rc : fail(front, rc, m->err);
  const tdt_buffer *cells = m->ssbo[TDT_SLOT_CELLS];
  if (cells->bytes > 0xFFFFFFF8ull)
    return fail(front, TDT_ERR_INVALID_VALUE, "cells buffer larger than 4 GiB is not addressable by the shader's 32-bit offsets");
  P.cells = (const uint32_t *)cells->dev; P.cells_dwords = (uint32_t)(cells->bytes >> 2);
  return TDT_OK;
}

// grow-only staging on the member context
int query_scratch(tdt_ctx *front, tdt_ctx *m, size_t bytes, void **out) {
  if (m->query_bytes < bytes) {
    if (m->query) (void)hipFree(m->query);
    m->query = nullptr; m->query_bytes = 0;
    const hipError_t e = hipMalloc(&m->query, bytes);
    if (e != hipSuccess) { m->query = nullptr; return hip_fail(front, e, "hipMalloc (ray query staging)"); }
    m->query_bytes = bytes;
  }
  *out = m->query;
  return TDT_OK;
}

template <bool PICK>
int launch_queries(tdt_ctx *front, tdt_ctx *m, const TraceParams &P, const float *rays, const int32_t *xy, int sample, float *rays_out,
                   void *hits, size_t n) {
  for (size_t b = 0; b < n; b += kQueryChunk) {
    const uint32_t k = (uint32_t)(n - b < kQueryChunk ? n - b : kQueryChunk);
    hipLaunchKernelGGL(raycast_kernel<PICK>, dim3((k + kQueryBlock - 1) / kQueryBlock), dim3(kQueryBlock), 0, m->stream, P,
                       PICK ? nullptr : rays + 6 * b, PICK ? xy + 2 * b : nullptr, sample, rays_out ? rays_out + 6 * b : nullptr,
                       static_cast<QueryOut *>(hits) + b, k);
  }
  TDT_HIP(front, hipGetLastError());
  return TDT_OK;
}

}  // namespace

void query_scratch_destroy(tdt_ctx *ctx) {
  if (ctx->query) (void)hipFree(ctx->query);
  ctx->query = nullptr; ctx->query_bytes = 0;
}

}  // namespace tdt

extern "C" {

int tdt_raycast(tdt_ctx *ctx, const float *rays, size_t n, tdt_ray_hit *out) {
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (n == 0) return TDT_OK;
  if (!rays || !out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null rays / out pointer");
  tdt_ctx *m = tdt::first_member(ctx);   // (its slots hold the replicas of the bound buffers)
  TraceParams P;
  if (int rc = tdt::query_params(ctx, m, P)) return rc;
  if (n > (~size_t(0)) / 128) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "too many rays");
  TDT_HIP(ctx, hipSetDevice(m->device));
  void *scratch = nullptr;
  if (int rc = tdt::query_scratch(ctx, m, n * (24 + sizeof(tdt_ray_hit)), &scratch)) return rc;
  void *d_hits = scratch;                                       // (the hits first: they are stored as 16-byte words)
  float *d_rays = reinterpret_cast<float *>(static_cast<char *>(scratch) + n * sizeof(tdt_ray_hit));
  TDT_HIP(ctx, hipMemcpyAsync(d_rays, rays, n * 24, hipMemcpyHostToDevice, m->stream));
  if (int rc = tdt::launch_queries<false>(ctx, m, P, d_rays, nullptr, 0, nullptr, d_hits, n)) return rc;
  TDT_HIP(ctx, hipMemcpyAsync(out, d_hits, n * sizeof(tdt_ray_hit), hipMemcpyDeviceToHost, m->stream));
  TDT_HIP(ctx, hipStreamSynchronize(m->stream));
  return TDT_OK;
}

int tdt_raycast_device(tdt_ctx *ctx, const void *rays_dev, size_t n, void *hits_dev) {
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (n == 0) return TDT_OK;
  if (!rays_dev || !hits_dev) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null rays / hits pointer");
  if (((uintptr_t)rays_dev & 3u) || ((uintptr_t)hits_dev & 15u))
    return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "rays must be 4-byte and hits 16-byte aligned");
  tdt_ctx *m = tdt::first_member(ctx);   // (its slots hold the replicas of the bound buffers)
  TraceParams P;
  if (int rc = tdt::query_params(ctx, m, P)) return rc;
  TDT_HIP(ctx, hipSetDevice(m->device));
  return tdt::launch_queries<false>(ctx, m, P, static_cast<const float *>(rays_dev), nullptr, 0, nullptr, hits_dev, n);
}

int tdt_pick_pixels(tdt_compute *c, const int32_t *xy, size_t n, int sample, float *rays_out, tdt_ray_hit *out) {
  if (!c) return TDT_ERR_INVALID_VALUE;
  tdt_ctx *ctx = c->ctx;
  if (c->kind != TDT_PROGRAM_RAYTRACER) return tdt::fail(ctx, TDT_ERR_INVALID_OPERATION, "pick needs a raytracer program (its camera)");
  if (n == 0) return TDT_OK;
  if (!xy || !out) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "null xy / out pointer");
  if (sample < 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "negative sample index");
  for (size_t i = 0; i < 2 * n; i++)
    if (xy[i] < 0) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "negative pixel coordinate");
  const tdt_compute *cam = c->replicas.empty() ? c : c->replicas[0];     // (a multi-device program: its first member's camera)
  tdt_ctx *m = cam->ctx;
  TraceParams P;
  if (int rc = tdt::query_params(ctx, m, P)) return rc;
  if (n > (~size_t(0)) / 128) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "too many rays");
  P.image_width = cam->image_width; P.image_height = cam->image_height;
  for (int i = 0; i < 3; i++) {
    P.hor[i] = cam->horizontal[i]; P.ver[i] = cam->vertical[i]; P.llc[i] = cam->lower_left_corner[i]; P.org[i] = cam->origin[i];
  }
  P.samples_per_pixel = cam->samples_per_pixel; P.max_bounce = cam->max_bounce;
  TDT_HIP(ctx, hipSetDevice(m->device));
  // staging: hits (16-byte aligned at the start), then the pixel pairs, then the rays
  const size_t hit_bytes = n * sizeof(tdt_ray_hit), xy_bytes = n * 8, ray_bytes = rays_out ? n * 24 : 0;
  void *scratch = nullptr;
  if (int rc = tdt::query_scratch(ctx, m, hit_bytes + xy_bytes + ray_bytes, &scratch)) return rc;
  char *base = static_cast<char *>(scratch);
  int32_t *d_xy = reinterpret_cast<int32_t *>(base + hit_bytes);
  float *d_rays = rays_out ? reinterpret_cast<float *>(base + hit_bytes + xy_bytes) : nullptr;
  TDT_HIP(ctx, hipMemcpyAsync(d_xy, xy, xy_bytes, hipMemcpyHostToDevice, m->stream));
  if (int rc = tdt::launch_queries<true>(ctx, m, P, nullptr, d_xy, sample, d_rays, base, n)) return rc;
  TDT_HIP(ctx, hipMemcpyAsync(out, base, hit_bytes, hipMemcpyDeviceToHost, m->stream));
  if (rays_out) TDT_HIP(ctx, hipMemcpyAsync(rays_out, d_rays, ray_bytes, hipMemcpyDeviceToHost, m->stream));
  TDT_HIP(ctx, hipStreamSynchronize(m->stream));
  return TDT_OK;
}

}  // extern "C"
