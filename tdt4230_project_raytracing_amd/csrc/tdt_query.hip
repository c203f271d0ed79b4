// Ray queries — "what is under this pixel?" (include/tdt_rt.h, tdt_raycast / tdt_raycast_device / tdt_pick_pixels).
//
// One query ray per lane runs OctreeHit (rc:397-450) as the trace kernel's general build runs it for a fresh invocation
// (zeroed Carry): root slab test, restart-from-root loop, the literal treeLookup (the float formula: right for every
// cell_count), the padded empty-cell exit and the i > 0 leaf slab test with its fall-back to the call site's old
// temporaries.  The traversal itself is query_first_hit (query_device.hpp), which the guide kernel (tdt_denoise.hip) runs too.
#include <cstring>
#include <new>
#include <string>

#include "tdt_internal.hpp"
#include "query_device.hpp"

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
  const NodeSource ns = query_node_source(P, s_escape);

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

  const QueryRecord q = query_first_hit(P, ns, r);
  QueryOut o;
  o.q[0] = make_uint4((uint32_t)q.status, q.material, __float_as_uint(q.t), (uint32_t)q.lookups);
  o.q[1] = make_uint4(__float_as_uint(q.rec.px), __float_as_uint(q.rec.py), __float_as_uint(q.rec.pz), __float_as_uint(q.rec.nx));
  o.q[2] = make_uint4(__float_as_uint(q.rec.ny), __float_as_uint(q.rec.nz), q.rec.ff ? 1u : 0u, q.fresh ? 1u : 0u);
  o.q[3] = make_uint4(__float_as_uint(q.cmin_x), __float_as_uint(q.cmin_y), __float_as_uint(q.cmin_z), __float_as_uint(q.csize));
  hits[i] = o;
}

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

// the camera uniforms of a program (primary_ray reads them)
void query_camera(const tdt_compute *cam, TraceParams &P) {
  P.image_width = cam->image_width; P.image_height = cam->image_height;
  for (int i = 0; i < 3; i++) {
    P.hor[i] = cam->horizontal[i]; P.ver[i] = cam->vertical[i]; P.llc[i] = cam->lower_left_corner[i]; P.org[i] = cam->origin[i];
  }
  P.samples_per_pixel = cam->samples_per_pixel; P.max_bounce = cam->max_bounce;
}

namespace {

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
  const tdt_compute *cam = tdt::camera_program(c);
  tdt_ctx *m = cam->ctx;
  TraceParams P;
  if (int rc = tdt::query_params(ctx, m, P)) return rc;
  if (n > (~size_t(0)) / 128) return tdt::fail(ctx, TDT_ERR_INVALID_VALUE, "too many rays");
  tdt::query_camera(cam, P);
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
