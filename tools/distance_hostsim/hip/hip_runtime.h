// host stand-in for the HIP constructs tdt_distance.hip uses: the enclosed-space unit's stand-in (one block at a time, 256 real
// threads behind a pthread barrier) plus the wave ballot, which every thread of the block calls together
#pragma once
#include "../../fill_hostsim/hip/hip_runtime.h"
inline unsigned long long __ballot(int p) {
  sim::slot[threadIdx.x] = p != 0;
  sim::sync();
  unsigned long long r = 0;
  const unsigned w = threadIdx.x & ~63u;
  for (unsigned i = 0; i < 64; i++) r |= (unsigned long long)sim::slot[w + i] << i;
  sim::sync();
  return r;
}
