// What the units that work on the tree's exposed faces share (tdt_surface.hip: the faces as quads; tdt_faces.hip: the faces
// labelled into face regions): the six-segment layout of a face array and the ONE definition of the face list — the walk, the
// keys, the exposed-face probe, the scan, the emit and the per-segment sort — which tdt_surface.hip owns and launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "region_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

struct SurfaceSegs { uint32_t at[7]; };                 // segment f = [at[f], at[f + 1]) of an array of at[6] items

__device__ __forceinline__ int surface_seg_of(const SurfaceSegs &s, uint32_t j) {
  int f = 0;
#pragma unroll
  for (int t = 1; t < 6; t++) f += j >= s.at[t] ? 1 : 0;
  return f;
}
__device__ __forceinline__ uint32_t surface_seg_start(const SurfaceSegs &s, uint32_t j) {   // at[surface_seg_of(j)], without indexing
  uint32_t lo = s.at[0];
#pragma unroll
  for (int t = 1; t < 6; t++) lo = j >= s.at[t] ? s.at[t] : lo;
  return lo;
}
__device__ __forceinline__ uint32_t surface_seg_end(const SurfaceSegs &s, uint32_t j) {     // at[surface_seg_of(j) + 1]
  uint32_t hi = s.at[6];
#pragma unroll
  for (int t = 5; t >= 1; t--) hi = j < s.at[t] ? s.at[t] : hi;
  return hi;
}

// The exposed faces of one single-device context's tree, everything in device memory of ctx allocated in S.
struct SurfaceFaces {
  int4 *v = nullptr; uint32_t nv = 0; int depth = 0;     // the tree's voxel list (null when nv == 0)
  uint32_t *keys = nullptr;                              // its Morton keys
  SurfaceSegs segs = {};                                 // the faces of direction f: [segs.at[f], segs.at[f + 1])
  uint32_t nf = 0;                                       // segs.at[6]
  // the faces, every segment sorted by key (null when nf == 0).  stacked = 1: (w << 20 | u << 10 | v, u << 8 | carried material),
  // the order of tdt_octree_extract_surface with merge = 0; stacked = 0: (w << 20 | v << 10 | u, carried material)
  uint32_t *fk = nullptr, *fv = nullptr;
  uint32_t *fk_alt = nullptr, *fv_alt = nullptr;         // a second pair of nf words, free after the sort
  uint32_t *hist = nullptr, *hscr = nullptr;             // the sorts' scratch, sized for the largest segment
  uint32_t *d_bounds = nullptr;                          // seven device words
};
// walk (tree_voxels_capped), keys, probe under the mask `shapes`, scan, emit, sort.  Queued on ctx's stream; host
// synchronisations: tree_voxels' own and ONE for the segment bounds.  Errors are reported on `front`.
int surface_face_list(tdt_ctx *front, tdt_ctx *ctx, const std::vector<RegionShape> &shapes, int by_material, int stacked, DeviceScratch &S,
                      SurfaceFaces &F);
// the n faces of a stacked list as 1 x 1 tdt_quads (two int4 each) into quads, queued on st
void surface_unit_quads(hipStream_t st, const uint32_t *fk, const uint32_t *fv, uint32_t n, const SurfaceSegs &segs, int4 *quads);

}  // namespace tdt
