// Device helpers of the dense bit volumes that enclosed space (tdt_fill.hip), exact Euclidean distance (tdt_distance.hip),
// affine transforms (tdt_xform.hip) and geodesic distance (tdt_geodesic.hip) keep over a box of the grid, and the host steps
// around a unit's own kernels (at the end); the kernels and the other host steps they share are tdt_bitvol.hip's.
//
// The layout: x runs along the 32-bit word.  A row (y, z) of the box is nw <= 32 consecutive words, word w of a row holding
// x = 32 (wx0 + w) .. + 31, so rows are word-aligned in ABSOLUTE x and the box itself need not be: the bits of a row's first
// and last word that lie outside [lo[0], hi[0]] are masked (bitvol_valid).  Rows follow each other in y, then in z:
// word g = ((z - lo[2]) * ey + (y - lo[1])) * nw + w.
#pragma once
#include <string>

#include "region_device.hpp"

namespace tdt {

// device_scan.hpp's, which a unit that calls bitvol_list_tail includes (its kernels are compiled into every unit that does:
// tdt_bitvol.hip has no use for them)
inline size_t scan_scratch_words(size_t n);
inline hipError_t exclusive_scan_u32(hipStream_t stream, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *scratch);

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

// ---- host steps that run a unit's own kernels (templates over what queues them; the rest is tdt_bitvol.hip's).  Everything is
// queued on `st`; errors are reported on `front` ----
constexpr int kBitvolBatch = 8;                              // passes per flag read

// A fixed point by passes: pass(flag) queues one pass, which raises *flag when it changed the volume.  Batches of kBitvolBatch
// passes, each with a flag word of its own (flags: kBitvolBatch words), read with ONE synchronisation per batch, until the last
// pass of a batch changed nothing: at most kBitvolBatch - 1 passes run idle.  *last (zeroed by the caller) = the number of the
// last pass that changed the volume.
template <class Pass> int bitvol_pass_loop(tdt_ctx *front, hipStream_t st, uint32_t *flags, Pass &&pass, uint32_t *last) {
  uint32_t h_flags[kBitvolBatch], queued = 0;
  do {
    TDT_HIP(front, hipMemsetAsync(flags, 0, sizeof h_flags, st));
    for (int p = 0; p < kBitvolBatch; p++) pass(flags + p);
    TDT_HIP(front, hipGetLastError());
    TDT_HIP(front, hipMemcpyAsync(h_flags, flags, sizeof h_flags, hipMemcpyDeviceToHost, st));
    TDT_HIP(front, hipStreamSynchronize(st));              // one per batch of passes
    for (int p = kBitvolBatch - 1; p >= 0; p--)
      if (h_flags[p]) { *last = queued + (uint32_t)p + 1u; break; }
    queued += kBitvolBatch;
  } while (h_flags[kBitvolBatch - 1]);
  return TDT_OK;
}

// The tail of a unit's list: count(count) queues the kernel that writes the selected bits of each of n_items items (words, or
// a brick's words) and 0 into the extra item count[n_items]; the scan leaves the total there, which is read (the ONE
// synchronisation before the emit) and held to kBitvolCap ("<noun> holds N voxels"); emit(excl, keys, vals) queues the
// kernel that writes (Morton key, material + 1) per selected bit at its item's offset; bitvol_emit_list ends it.  n_head ready
// pairs (head_k / head_v, not under the cap) go in front of the emitted ones.  *out = *n voxels in S; the caller has set null / 0.
template <class Count, class Emit>
int bitvol_list_tail(tdt_ctx *front, hipStream_t st, size_t n_items, Count &&count_kernel, Emit &&emit_kernel, const char *noun, bool sort,
                     const uint32_t *head_k, const uint32_t *head_v, uint32_t n_head, DeviceScratch &S, const char *no_memory, const int4 **out,
                     uint32_t *n) {
  uint32_t *count = S.get<uint32_t>(n_items + 1), *scr = S.get<uint32_t>(scan_scratch_words(n_items + 1));
  if (!count || !scr) return fail(front, TDT_ERR_HIP, no_memory);
  count_kernel(count);
  TDT_HIP(front, exclusive_scan_u32(st, count, count, (uint32_t)(n_items + 1), scr));
  TDT_HIP(front, hipGetLastError());
  uint32_t n_sel = 0;                                      // <= 2^30 in every unit
  if (int rc = read_word(front, st, count + n_items, &n_sel)) return rc;   // the count
  if (n_sel > kBitvolCap)
    return fail(front, TDT_ERR_INVALID_VALUE, std::string(noun) + " holds " + std::to_string(n_sel) + " voxels (more than 2^26)");
  const uint32_t n_out = n_sel + n_head;
  if (n_out == 0) return TDT_OK;
  uint32_t *k0 = S.get<uint32_t>(n_out), *v0 = S.get<uint32_t>(n_out);
  if (!k0 || !v0) return fail(front, TDT_ERR_HIP, no_memory);
  if (n_head) {
    TDT_HIP(front, hipMemcpyAsync(k0, head_k, (size_t)n_head * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    TDT_HIP(front, hipMemcpyAsync(v0, head_v, (size_t)n_head * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  }
  if (n_sel) emit_kernel((const uint32_t *)count, k0 + n_head, v0 + n_head);
  if (int rc = bitvol_emit_list(front, st, k0, v0, n_out, sort, S, no_memory, out)) return rc;
  *n = n_out;
  return TDT_OK;
}

// A field request's box lo..hi, on the host: inside the grid of side 2^depth and held to kBitvolCap voxels; then domain(), what
// else of the request the host can refuse before the count is given; then *n_voxels = the box's voxels and, when the field is
// wanted, the capacity check.  Nothing is queued, so the count-only call costs no tree walk.
template <class Domain>
int bitvol_field_box(tdt_ctx *front, int depth, const int32_t lo[3], const int32_t hi[3], Domain &&domain, bool wanted, size_t capacity,
                     size_t *n_voxels) {
  unsigned long long count = 1;
  for (int a = 0; a < 3; a++) {
    if (lo[a] < 0 || hi[a] >= (1 << depth) || lo[a] > hi[a]) return fail(front, TDT_ERR_INVALID_VALUE, "the box must satisfy 0 <= lo <= hi < 2^max_depth");
    count *= (unsigned long long)(hi[a] - lo[a] + 1);
  }
  if (count > kBitvolCap) return fail(front, TDT_ERR_INVALID_VALUE, "the box holds " + std::to_string(count) + " voxels (more than 2^26)");
  if (int rc = domain()) return rc;
  *n_voxels = (size_t)count;
  if (wanted && capacity < count) return fail(front, TDT_ERR_INVALID_VALUE, "capacity " + std::to_string(capacity) + " < " + std::to_string(count) + " voxels");
  return TDT_OK;
}

}  // namespace tdt
