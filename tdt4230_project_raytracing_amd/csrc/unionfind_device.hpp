// The lock-free union-find of the labelling units (tdt_connect.hip: voxels into components; tdt_faces.hip: exposed faces into
// face regions), and the run arithmetic of their in-wave reductions.  parent[i] <= i always: the larger root is hung under the
// smaller one by atomicCAS, so the final root of every set is its lowest index whatever the schedule.  Parent words are read with
// agent-scope relaxed atomic loads (a plain load may be served by the CU's non-coherent L1 and see a stale root) and path halving
// writes them with agent-scope atomic stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tdt {

__device__ __forceinline__ uint32_t uf_load(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, halving the path on the way (every parent word is an ancestor with a lower index, so any value a racing
// store leaves there is still one)
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t px = uf_load(parent + x);
    if (px == x) return x;
    const uint32_t gx = uf_load(parent + px);
    if (gx == px) return px;
    __hip_atomic_store(parent + x, gx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gx;
  }
}

__device__ __forceinline__ void uf_unite(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }     // hang the larger root under the smaller one
    if (atomicCAS(parent + a, a, b) == a) return;
  }
}

// the lane of the first lane of this lane's run (heads: one bit per lane that starts a run; lane 0 always does)
__device__ __forceinline__ uint32_t run_head(unsigned long long heads, uint32_t lane) {
  const unsigned long long upto = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);
  return 63u - (uint32_t)__clzll(heads & upto);
}

// root[i] = the root of i; flag[i] = i is a root; flag[n] = 0 (an exclusive scan over n + 1 leaves the count in [n]).  Queued on
// st (tdt_connect.hip)
void connect_flatten(hipStream_t st, uint32_t *parent, uint32_t n, uint32_t *root, uint32_t *flag);

}  // namespace tdt
