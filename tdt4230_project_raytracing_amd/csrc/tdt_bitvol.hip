// The dense bit volume over a box of the grid that enclosed space (tdt_fill.hip), exact Euclidean distance (tdt_distance.hip),
// affine transforms (tdt_xform.hip) and geodesic distance (tdt_geodesic.hip) share: the steps that take the tree's
// Morton-sorted voxel list into the volume and a selection of its bits back into a list.  The layout, the device helpers of
// the units' own count and emit kernels, and the host steps around those kernels (the pass loop, the list's tail from the
// count to the list, a field's box: templates over what queues the unit's kernel) are bitvol_device.hpp's; the declarations
// are in tdt_internal.hpp.  A kernel is launched from the unit that defines it, so the kernels here are reached through the
// host functions below only.
//
//   bbox       one reduction over the list: a fixed launch of at most 256 blocks whose lanes stride over the list, wave
//              shuffles, then one vector atomicMin / atomicMax per wave and axis: at most 6144 per call, on integers, so the
//              result does not depend on their order; a second reduction kernel over per-wave partials would add a launch to
//              save them.  (One wave per 64 voxels measured 1.0 ms on config 3's 0.95 M voxels: 90 000 atomics on six
//              words.)                                                                                    bitvol_bbox_kernel
//   rasterise  one lane per voxel of the list: its (Morton key, material + 1) for the material lookups, and, when it lies
//              inside the box, a vector atomicOr of its bit into the occupancy volume.               bitvol_rasterise_kernel
//   list       after the unit's emit kernel has written (Morton key, material + 1) per selected bit: the builder's radix sort
//              where the order matters, then one lane per pair writes {x, y, z, m}.                       bitvol_list_kernel
#include <climits>

#include "bitvol_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr unsigned kBboxBlocks = 256;                    // the bounding box's launch: 1024 waves, 6 atomics each

// box[0..2] = min, box[3..5] = max over the list (initialised to INT_MAX / -1)
// A lane takes every stride-th voxel (stride = the launch's lanes, a multiple of 64, so a wave's trip counts differ by one at
// most and all its lanes reach the shuffles): the atomics per call are bounded by the launch, not by the list.
__global__ __launch_bounds__(256) void bitvol_bbox_kernel(const int4 *v, uint32_t n, uint32_t stride, int *box) {
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const int4 p = v[i];
    lo[0] = p.x < lo[0] ? p.x : lo[0]; lo[1] = p.y < lo[1] ? p.y : lo[1]; lo[2] = p.z < lo[2] ? p.z : lo[2];
    hi[0] = p.x > hi[0] ? p.x : hi[0]; hi[1] = p.y > hi[1] ? p.y : hi[1]; hi[2] = p.z > hi[2] ? p.z : hi[2];
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int l = bitvol_wave_min(lo[a]), h = -bitvol_wave_min(-hi[a]);
    if ((threadIdx.x & 63u) == 0 && h >= 0) { atomicMin(box + a, l); atomicMax(box + 3 + a, h); }
  }
}

__global__ __launch_bounds__(256) void bitvol_rasterise_kernel(const int4 *v, uint32_t n, const BitBox B, uint32_t *occ, uint32_t *keys,
                                                              uint32_t *vals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 p = v[i];
  keys[i] = region_key(p.x, p.y, p.z);
  vals[i] = (uint32_t)p.w;
  if (p.x < B.lo[0] || p.x > B.hi[0] || p.y < B.lo[1] || p.y > B.hi[1] || p.z < B.lo[2] || p.z > B.hi[2]) return;
  const uint32_t row = (uint32_t)(p.z - B.lo[2]) * (uint32_t)B.ey + (uint32_t)(p.y - B.lo[1]);
  atomicOr(occ + row * (uint32_t)B.nw + (uint32_t)((p.x >> 5) - B.wx0), 1u << (p.x & 31));
}

__global__ __launch_bounds__(256) void bitvol_list_kernel(const uint32_t *keys, const uint32_t *vals, uint32_t n, int4 *out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  out[i] = region_voxel(keys[i], (int)vals[i]);
}

void bitvol_layout(const int lo[3], const int hi[3], BitBox &B) {
  for (int a = 0; a < 3; a++) { B.lo[a] = lo[a]; B.hi[a] = hi[a]; }
  B.ey = B.hi[1] - B.lo[1] + 1; B.ez = B.hi[2] - B.lo[2] + 1;
  B.wx0 = B.lo[0] >> 5; B.nw = (B.hi[0] >> 5) - B.wx0 + 1;
  B.n_words = (uint32_t)B.ey * (uint32_t)B.ez * (uint32_t)B.nw;
}

int bitvol_list_bbox(tdt_ctx *front, hipStream_t st, const int4 *v, uint32_t n, int depth, DeviceScratch &S, const char *no_memory,
                     const char *outside, int box[6]) {
  const int init[6] = {INT_MAX, INT_MAX, INT_MAX, -1, -1, -1};
  int *d_box = S.get<int>(6);
  if (!d_box) return fail(front, TDT_ERR_HIP, no_memory);
  TDT_HIP(front, hipMemcpyAsync(d_box, init, sizeof init, hipMemcpyHostToDevice, st));
  const unsigned bbox_blocks = blocks_of(n) < kBboxBlocks ? blocks_of(n) : kBboxBlocks;
  hipLaunchKernelGGL(bitvol_bbox_kernel, dim3(bbox_blocks), dim3(256), 0, st, v, n, bbox_blocks * 256u, d_box);
  TDT_HIP(front, hipGetLastError());
  TDT_HIP(front, hipMemcpyAsync(box, d_box, 6 * sizeof(int), hipMemcpyDeviceToHost, st));
  TDT_HIP(front, hipStreamSynchronize(st));                // the box sizes the volumes
  const int N = 1 << depth;
  for (int a = 0; a < 3; a++)
    if (box[a] < 0 || box[3 + a] >= N || box[a] > box[3 + a]) return fail(front, TDT_ERR_INVALID_VALUE, outside);
  return TDT_OK;
}

int bitvol_rasterise(tdt_ctx *front, hipStream_t st, const int4 *v, uint32_t n, const BitBox &B, uint32_t *occ, uint32_t *keys, uint32_t *vals) {
  TDT_HIP(front, hipMemsetAsync(occ, 0, (size_t)B.n_words * sizeof(uint32_t), st));
  if (n) hipLaunchKernelGGL(bitvol_rasterise_kernel, dim3(blocks_of(n)), dim3(256), 0, st, v, n, B, occ, keys, vals);
  return TDT_OK;
}

int bitvol_emit_list(tdt_ctx *front, hipStream_t st, uint32_t *k, uint32_t *v, uint32_t n, bool sort, DeviceScratch &S, const char *no_memory,
                     const int4 **out) {
  int4 *vox = S.get<int4>(n);
  if (!vox) return fail(front, TDT_ERR_HIP, no_memory);
  if (sort) {
    uint32_t *k1 = S.get<uint32_t>(n), *v1 = S.get<uint32_t>(n);
    uint32_t *hist = S.get<uint32_t>(sort_hist_words(n)), *hscr = S.get<uint32_t>(sort_scratch_words(n));
    if (!k1 || !v1 || !hist || !hscr) return fail(front, TDT_ERR_HIP, no_memory);
    TDT_HIP(front, sort_pairs_u32(st, k, v, k1, v1, n, hist, hscr));
  }
  hipLaunchKernelGGL(bitvol_list_kernel, dim3(blocks_of(n)), dim3(256), 0, st, (const uint32_t *)k, (const uint32_t *)v, n, vox);
  TDT_HIP(front, hipGetLastError());
  TDT_HIP(front, hipStreamSynchronize(st));
  *out = vox;
  return TDT_OK;
}

}  // namespace tdt
