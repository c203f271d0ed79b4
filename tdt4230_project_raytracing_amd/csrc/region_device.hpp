// Device helpers shared by the editing units: Morton keys of grid voxels and a key's voxel, the exact integer shape test of a
// tdt_region, the lower- and upper-bound searches of the rank merges and the neighbour lookup in a sorted key list; and the two host steps every unit with a region list takes: the list's validation
// with its copy into RegionShapes, and their upload.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "tdt_internal.hpp"

namespace tdt {

struct RegionShape {           // a tdt_region with its grid-clipped bounding box (lo, ext) and first candidate lane
  int32_t shape, a[3], b[3];
  int32_t lo[3];
  uint32_t ext[3], lane0;
};

// a call's region list checked as every entry point checks it; out (may be null): the shapes, shape / a / b copied, the rest 0
inline int region_shapes(tdt_ctx *ctx, const tdt_region *regions, size_t n_regions, std::vector<RegionShape> *out) {
  if (n_regions && !regions) return fail(ctx, TDT_ERR_INVALID_VALUE, "null region list");
  if (out) out->assign(n_regions, RegionShape{});
  for (size_t s = 0; s < n_regions; s++) {
    const tdt_region &g = regions[s];
    if (g.shape != TDT_SHAPE_BOX && g.shape != TDT_SHAPE_SPHERE) return fail(ctx, TDT_ERR_INVALID_VALUE, "shape must be TDT_SHAPE_BOX or TDT_SHAPE_SPHERE");
    if (g.shape == TDT_SHAPE_SPHERE && g.b[0] < 0) return fail(ctx, TDT_ERR_INVALID_VALUE, "sphere radius must be >= 0");
    if (!out) continue;
    (*out)[s].shape = g.shape;
    for (int a = 0; a < 3; a++) { (*out)[s].a[a] = g.a[a]; (*out)[s].b[a] = g.b[a]; }
  }
  return TDT_OK;
}
// *d = n shapes in device memory of S, queued on st (null when n == 0); no_memory: the caller's out-of-memory text
inline int upload_shapes(tdt_ctx *front, hipStream_t st, DeviceScratch &S, const RegionShape *shapes, size_t n, const char *no_memory, RegionShape **d) {
  *d = n ? S.get<RegionShape>(n) : nullptr;
  if (!n) return TDT_OK;
  if (!*d) return fail(front, TDT_ERR_HIP, no_memory);
  TDT_HIP(front, hipMemcpyAsync(*d, shapes, n * sizeof(RegionShape), hipMemcpyHostToDevice, st));
  return TDT_OK;
}

constexpr uint32_t kDroppedKey = 0xFFFFFFFFu;   // key of a voxel outside the grid: sorts behind everything, and the unique drops it

__device__ __forceinline__ uint32_t region_spread3(uint32_t v) {   // 10 bits -> every third bit
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__device__ __forceinline__ uint32_t region_compact3(uint32_t v) {  // every third bit -> 10 bits
  v &= 0x09249249u;
  v = (v | (v >> 2)) & 0x030C30C3u;
  v = (v | (v >> 4)) & 0x0300F00Fu;
  v = (v | (v >> 8)) & 0x030000FFu;
  v = (v | (v >> 16)) & 0x000003FFu;
  return v;
}
__device__ __forceinline__ uint32_t region_key(int x, int y, int z) {
  return (region_spread3((uint32_t)x) << 2) | (region_spread3((uint32_t)y) << 1) | region_spread3((uint32_t)z);
}

// the shape predicate in exact integer arithmetic: box lo <= p <= hi; sphere |p - c|^2 <= r^2 (each |d| <= r first, so the
// sum of three squares <= 3 * 2^62 fits in 64 unsigned bits)
__device__ __forceinline__ bool region_inside(const RegionShape &s, int x, int y, int z) {
  if (s.shape == TDT_SHAPE_BOX)
    return x >= s.a[0] && x <= s.b[0] && y >= s.a[1] && y <= s.b[1] && z >= s.a[2] && z <= s.b[2];
  const long long r = s.b[0];
  const long long dx = (long long)x - s.a[0], dy = (long long)y - s.a[1], dz = (long long)z - s.a[2];
  if (dx > r || dx < -r || dy > r || dy < -r || dz > r || dz < -r) return false;
  const unsigned long long d2 = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy) + (unsigned long long)(dz * dz);
  return d2 <= (unsigned long long)(r * r);
}

// the voxel of Morton key k, with w = m
__device__ __forceinline__ int4 region_voxel(uint32_t k, int m) {
  return make_int4((int)region_compact3(k >> 2), (int)region_compact3(k >> 1), (int)region_compact3(k), m);
}

// the number of keys below k (lower) / at or below k (upper) in the sorted keys[0, n): the index of the first that is not
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *keys, uint32_t n, uint32_t k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] < k) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ uint32_t upper_bound_u32(const uint32_t *keys, uint32_t n, uint32_t k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] <= k) lo = mid + 1; else hi = mid; }
  return lo;
}
// index of key kn in keys[0, n), or -1: a gallop from i (keys[i] = k != kn) toward kn, then a binary search
__device__ __forceinline__ int gallop_find(const uint32_t *keys, int n, int i, uint32_t k, uint32_t kn) {
  if (kn > k) {
    int lo = i, hi = n;                                    // keys[lo] < kn <= keys[hi] (hi = n: past the end)
    for (int step = 1; step <= n - 1 - i; step <<= 1) {
      const int j = i + step;
      if (keys[j] >= kn) { hi = j; break; }
      lo = j;
      if (step > (INT_MAX >> 1)) break;
    }
    while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (keys[mid] < kn) lo = mid; else hi = mid; }
    return hi < n && keys[hi] == kn ? hi : -1;
  }
  int lo = -1, hi = i;                                     // keys[lo] <= kn < keys[hi] (lo = -1: before the start)
  for (int step = 1; step <= i; step <<= 1) {
    const int j = i - step;
    if (keys[j] <= kn) { lo = j; break; }
    hi = j;
    if (step > (INT_MAX >> 1)) break;
  }
  while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (keys[mid] <= kn) lo = mid; else hi = mid; }
  return lo >= 0 && keys[lo] == kn ? lo : -1;
}

}  // namespace tdt
