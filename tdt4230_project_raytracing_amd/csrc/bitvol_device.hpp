// Device helpers of the dense bit volumes that enclosed space (tdt_fill.hip) and exact Euclidean distance (tdt_distance.hip)
// keep over a box of the grid; the kernels and host steps both share are tdt_bitvol.hip's.
//
// The layout: x runs along the 32-bit word.  A row (y, z) of the box is nw <= 32 consecutive words, word w of a row holding
// x = 32 (wx0 + w) .. + 31, so rows are word-aligned in ABSOLUTE x and the box itself need not be: the bits of a row's first
// and last word that lie outside [lo[0], hi[0]] are masked (bitvol_valid).  Rows follow each other in y, then in z:
// word g = ((z - lo[2]) * ey + (y - lo[1])) * nw + w.
#pragma once
#include "region_device.hpp"

namespace tdt {

struct BitBox {                // a box of the grid and the layout of the bit volumes over it (bitvol_layout fills it)
  int32_t lo[3], hi[3];        // inclusive
  int32_t ey, ez;              // rows per axis
  int32_t nw, wx0;             // words per row; the absolute word index of word 0
  uint32_t n_words;            // ey * ez * nw <= 2^25
};

// the bits of word w of a row that lie inside [x0, x1]
__device__ __forceinline__ uint32_t bitvol_valid(const BitBox &B, int w) {
  uint32_t m = 0xFFFFFFFFu;
  if (w == 0) m &= 0xFFFFFFFFu << (B.lo[0] & 31);
  if (w == B.nw - 1) m &= 0xFFFFFFFFu >> (31 - (B.hi[0] & 31));
  return m;
}

// word g of a volume: its index in the row (returned), the x of its bit 0, its y and z
__device__ __forceinline__ int bitvol_word(const BitBox &B, uint32_t g, int *x0, int *y, int *z) {
  const int w = (int)(g % (uint32_t)B.nw);
  const uint32_t row = g / (uint32_t)B.nw;
  *x0 = (B.wx0 + w) << 5; *y = B.lo[1] + (int)(row % (uint32_t)B.ey); *z = B.lo[2] + (int)(row / (uint32_t)B.ey);
  return w;
}

// the bits of a word at (x0, y, z) that lie inside one of the shapes: the exact integer test of region edits per set bit
__device__ __forceinline__ uint32_t bitvol_inside(uint32_t bits, const RegionShape *shapes, uint32_t n_shapes, int x0, int y, int z) {
  uint32_t kept = 0;
  for (uint32_t b = bits; b; b &= b - 1u) {
    const int bit = __ffs((int)b) - 1;
    bool in = false;
    for (uint32_t s = 0; s < n_shapes && !in; s++) in = region_inside(shapes[s], x0 + bit, y, z);
    if (in) kept |= 1u << bit;
  }
  return kept;
}

// index of key k in the sorted keys[0, n) (k is there)
__device__ __forceinline__ uint32_t bitvol_find(const uint32_t *keys, uint32_t n, uint32_t k) {
  uint32_t lo = 0, hi = n;                                   // keys[lo] <= k < keys[hi]
  while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (keys[mid] <= k) lo = mid; else hi = mid; }
  return lo;
}

__device__ __forceinline__ int bitvol_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
  return v;
}

}  // namespace tdt
