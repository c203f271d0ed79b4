// Device helpers shared by region edits (tdt_region.hip), connected components (tdt_connect.hip) and voxel morphology
// (tdt_morph.hip): Morton keys of grid voxels, the exact integer shape test of a tdt_region, and the neighbour lookup in a
// sorted key list.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "tdt_rt.h"

namespace tdt {

struct RegionShape {           // a tdt_region with its grid-clipped bounding box (lo, ext) and first candidate lane
  int32_t shape, a[3], b[3];
  int32_t lo[3];
  uint32_t ext[3], lane0;
};

__device__ __forceinline__ uint32_t region_spread3(uint32_t v) {   // 10 bits -> every third bit (the builder's spread3)
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__device__ __forceinline__ uint32_t region_compact3(uint32_t v) {
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
