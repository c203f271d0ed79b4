// The Morton-sorted voxel list every editing unit starts from (tree_voxels, tdt_compact.hip), and the steps the list-based units
// take on it in the same form: the capped tree list, the keys of a list, the last-of-run flags and (key, value) unique behind a sort
// of pairs, and the scan-gather-count that closes a pass of keep flags.  The device helpers the units' own kernels call (the
// searches, the key's voxel, Morton arithmetic) are region_device.hpp's; the host helpers around a call (first member, the replicas'
// edit frame, the rebuild tail, the word read) and the declarations are tdt_internal.hpp's.  A kernel is launched from the unit that
// defines it, so the kernels here are reached through the host functions below only.
#include "device_scan.hpp"
#include "region_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

__global__ __launch_bounds__(256) void voxlist_keys_kernel(const int4 *v, uint32_t n, uint32_t *k) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) { const int4 p = v[i]; k[i] = region_key(p.x, p.y, p.z); }
}

// of every run of equal sorted keys keep the LAST (the stable sort kept list order: Grid::set overwrites); flag[n] = 0
__global__ __launch_bounds__(256) void voxlist_last_flags_kernel(const uint32_t *keys, uint32_t n, uint32_t *flag /* n + 1 */) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  flag[i] = (i < n && keys[i] != kDroppedKey && (i + 1u == n || keys[i + 1u] != keys[i])) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void voxlist_unique_kernel(const uint32_t *keys, const uint32_t *vals, uint32_t n, const uint32_t *excl /* n + 1 */,
                                                             uint32_t *uk, uint32_t *uv, uint32_t *count) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) *count = excl[n];
  if (i >= n) return;
  if (excl[i + 1u] != excl[i]) { uk[excl[i]] = keys[i]; uv[excl[i]] = vals[i]; }
}

// the kept voxels, and their keys where k is given, in order
__global__ __launch_bounds__(256) void voxlist_gather_kernel(const int4 *v, const uint32_t *k, const uint32_t *excl, uint32_t n, int4 *ov,
                                                             uint32_t *ok) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || excl[i + 1u] == excl[i]) return;
  ov[excl[i]] = v[i];
  if (ok) ok[excl[i]] = k[i];
}

int voxlist_within_cap(tdt_ctx *front, uint32_t n) {
  if (n > kVoxelListCap) return fail(front, TDT_ERR_INVALID_VALUE, "the tree holds " + std::to_string(n) + " voxels (more than 2^26)");
  return TDT_OK;
}

int tree_voxels_capped(tdt_ctx *front, tdt_ctx *ctx, DeviceScratch &S, int4 **out, uint32_t *n, int *depth) {
  if (int rc = tree_voxels(front, ctx, 254u, S, out, n, depth)) return rc;
  return voxlist_within_cap(front, *n);
}

void voxlist_keys(hipStream_t st, const int4 *v, uint32_t n, uint32_t *k) {
  hipLaunchKernelGGL(voxlist_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, st, v, n, k);
}

void voxlist_last_flags(hipStream_t st, const uint32_t *keys, uint32_t n, uint32_t *flag) {
  hipLaunchKernelGGL(voxlist_last_flags_kernel, dim3(blocks_of((size_t)n + 1)), dim3(256), 0, st, keys, n, flag);
}
void voxlist_unique(hipStream_t st, const uint32_t *keys, const uint32_t *vals, uint32_t n, const uint32_t *excl, uint32_t *uk, uint32_t *uv,
                    uint32_t *count) {
  hipLaunchKernelGGL(voxlist_unique_kernel, dim3(blocks_of(n)), dim3(256), 0, st, keys, vals, n, excl, uk, uv, count);
}

int scan_gather_count(tdt_ctx *front, hipStream_t st, const int4 *v, const uint32_t *k, uint32_t *keep, uint32_t n, uint32_t *scr, int4 *ov,
                      uint32_t *ok, uint32_t *total) {
  TDT_HIP(front, exclusive_scan_u32(st, keep, keep, n + 1u, scr));
  hipLaunchKernelGGL(voxlist_gather_kernel, dim3(blocks_of(n)), dim3(256), 0, st, v, k, (const uint32_t *)keep, n, ov, ok);
  TDT_HIP(front, hipGetLastError());
  return read_word(front, st, keep + n, total);
}

}  // namespace tdt
