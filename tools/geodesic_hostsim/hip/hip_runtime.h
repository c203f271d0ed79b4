// host stand-in for the HIP constructs tdt_geodesic.hip uses: exactly the transform unit's (one block at a time, real threads
// behind a pthread barrier, the block-wide or, the wave ballot)
#pragma once
#include "../../xform_hostsim/hip/hip_runtime.h"
