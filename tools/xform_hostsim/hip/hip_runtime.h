// host stand-in for the HIP constructs tdt_xform.hip uses: the distance unit's stand-in (one block at a time, 256 real threads
// behind a pthread barrier, the wave ballot) plus the 64-bit population count
#pragma once
#include "../../distance_hostsim/hip/hip_runtime.h"
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
