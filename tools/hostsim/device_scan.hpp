#pragma once
#include <hip/hip_runtime.h>
namespace tdt {
inline size_t scan_scratch_words(size_t) { return 1; }
inline hipError_t exclusive_scan_u32(hipStream_t, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *) {
  uint32_t s = 0; for (uint32_t i = 0; i < n; i++) { const uint32_t t = in[i]; out[i] = s; s += t; } return 0;
}
}
