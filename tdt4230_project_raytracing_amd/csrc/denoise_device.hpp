// What the image filters share on the device (tdt_denoise.hip, tdt_variance.hip, tdt_reproject.hip): the tile of a block, the
// surface key of a guide texel and its comparison, and the luminance the variance units measure.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "trace_device.hpp"

namespace tdt {

constexpr int kTileW = 32, kTileH = 8;               // pixels of a block, one per lane
constexpr int kMaxPasses = 8;

// words 0, 1, 2 of a guide texel; w = 1 marks a texel inside the image (outside: all four zero, which matches no centre)
TDT_DEV uint4 key_of(const uint4 g) { return make_uint4(g.x, g.y, g.z, 1u); }
TDT_DEV bool same_key(const uint4 a, const uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

TDT_DEV void tile_origin(uint32_t tiles_x, int &x0, int &y0) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  x0 = (int)tx * kTileW; y0 = (int)ty * kTileH;
}

// three multiplies and two adds, unfused (the build's parity flags)
TDT_DEV float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

}  // namespace tdt
