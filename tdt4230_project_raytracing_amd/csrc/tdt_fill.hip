// Enclosed space (include/tdt_rt.h tdt_octree_extract_enclosed / tdt_octree_fill_enclosed / tdt_voxelize_triangles_solid /
// tdt_octree_edit_triangles_solid): E(W, c), the EMPTY voxels of the grid [0, 2^depth)^3 that no path through empty
// c-neighbours connects to a face of the grid, W being the bound tree's voxels or a mesh's surface voxels.
//
// Every other editing unit works on the Morton-sorted list of OCCUPIED voxels; enclosure is a property of the empty ones, which
// are in no list, so this unit keeps a dense bit volume instead (layout: bitvol_device.hpp; the steps between the list and the
// volume that exact distance takes too: tdt_bitvol.hip).  It only has to span bbox(W): a voxel outside the bounding box
// of W is beyond it on some axis, walking away from the box along that axis stays empty up to the grid face, so every voxel
// outside bbox(W) is outside and E lies inside bbox(W).  An empty voxel on one of the six faces of bbox(W) is either on a grid
// face or next to a voxel outside the box: those are the seeds, and the flood never has to leave the box.
//
//   bbox, rasterise   tdt_bitvol.hip's: bbox(W) in its bounded launch, then W's occupancy bits and its (Morton key, material + 1);
//              the box being W's own, the rasteriser's clip never fires.
//   seed       reach = the empty bits of the rows on the four y / z faces, and the bits x0 and x1 of every other row.  fill_seed_kernel
//   flood      one block owns a tile of 8 x 8 whole rows, held in LDS with a halo of one row all round (10 x 10 rows); a tile
//              holds its rows whole, so there is no halo along x.  A round computes, per word,
//                reach |= fill(empty, empty & (carry bits of the row's neighbouring words | the 4 face rows (connectivity 6)
//                                               or the 8 rows around it, each spread by +-1 bit across words (connectivity 26)))
//              where fill() floods every run of empties that holds a seed bit in O(1) word operations: e & ~(e + s) | s carries
//              a seed upwards to the end of its run, the same on the bit-reversed words carries it downwards.  Rounds repeat
//              inside the tile until __syncthreads_or reports no change; then the tile's words are written back and, if any
//              changed, the pass's flag word is raised.                                                       fill_flood_kernel
//              Bits are only ever set, and a word of the volume is written by the one block that owns its row, with a plain
//              store of a superset of what it loaded; a block that reads a neighbour's row for its halo while that neighbour
//              writes it sees, word by word, the old or the new value, both subsets of the fixed point, so a half-updated
//              volume is harmless.  A pass whose flag stays clear changed nothing anywhere, so every block saw the final volume
//              and found its tile stable: that is the fixed point.
//              Passes: information crosses one tile boundary per pass at least, so the number of passes is bounded by 1 + the
//              length, in tiles entered, of the longest shortest path from a seed through empties (the longest corridor).  The
//              host queues them in batches with one flag read per batch (bitvol_pass_loop).
//   count      per word popc(empty & ~reach & in-mask), the mask being the exact integer test of region edits per set bit;
//              bitvol_list_tail scans the counts, reads the total (one synchronisation) and holds it to 2^26.  fill_count_kernel
//   emit       (Morton key, material + 1) per enclosed voxel at its word's offset.  Inherit: the first voxel of W in decreasing
//              x is the highest set occupancy bit below the voxel, in its word (a count of leading zeros) or the words before
//              it — it exists, or the voxel would reach the box's x0 face and be a seed — and its material is looked up in W's
//              sorted keys.  tdt_bitvol.hip's tail then sorts the pairs (W's own pairs in front of them for the solid mesh
//              forms) and writes the list {x, y, z, m}.                                                       fill_emit_kernel
//   memory     at the largest box (depth 10, the whole grid: 2^25 words): occupancy 128 MiB + reach 128 MiB + the per-word counts
//              and their scan 128 MiB (+ 64 KiB of scan scratch), besides W's list (16 B per voxel) and its (key, material)
//              pairs (8 B), and 32 B per resulting voxel for the pairs, the sort's second pair and the list.
#include <string>
#include <vector>

#include "bitvol_device.hpp"
#include "device_scan.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr int kFillTile = 8;                           // rows per tile side, in y and in z
constexpr int kFillHalo = kFillTile + 2;
constexpr int kFillMaxWords = 32;                      // words per row: 2^10 voxels / 32

// every run of set bits of e that holds a bit of s (s a subset of e), whole.  e + s: the lowest seed of a run carries through
// the run's bits above it and stops in the clear bit behind the run (or leaves the word); a higher seed of the same run stays
// set in the sum, hence the final | s.
__device__ __forceinline__ uint32_t fill_runs(uint32_t e, uint32_t s) {
  const uint32_t up = (e & ~(e + s)) | s;
  const uint32_t eb = __brev(e), sb = __brev(s);
  return up | __brev((eb & ~(eb + sb)) | sb);
}

__global__ __launch_bounds__(256) void fill_seed_kernel(const BitBox B, const uint32_t *occ, uint32_t *reach) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= B.n_words) return;
  const int w = (int)(g % (uint32_t)B.nw);
  const uint32_t row = g / (uint32_t)B.nw;
  const int y = (int)(row % (uint32_t)B.ey), z = (int)(row / (uint32_t)B.ey);
  const uint32_t empty = ~occ[g] & bitvol_valid(B, w);
  uint32_t seed = 0xFFFFFFFFu;
  if (y != 0 && y != B.ey - 1 && z != 0 && z != B.ez - 1) {
    seed = 0;
    if (w == 0) seed |= 1u << (B.lo[0] & 31);
    if (w == B.nw - 1) seed |= 1u << (B.hi[0] & 31);
  }
  reach[g] = empty & seed;
}

// r: the halo'd tile's reach words, row-major; the word w of row h spread by one bit either way, across its neighbouring words
__device__ __forceinline__ uint32_t fill_spread(const uint32_t *r, int h, int w, int nw) {
  const uint32_t c = r[h * nw + w];
  uint32_t s = c | (c << 1) | (c >> 1);
  if (w > 0) s |= r[h * nw + w - 1] >> 31;
  if (w < nw - 1) s |= r[h * nw + w + 1] << 31;
  return s;
}

template <int CONN>
__global__ __launch_bounds__(256) void fill_flood_kernel(const BitBox B, const uint32_t *occ, uint32_t *reach, uint32_t *flag) {
  __shared__ uint32_t r[kFillHalo * kFillHalo * kFillMaxWords];
  __shared__ uint32_t e[kFillTile * kFillTile * kFillMaxWords];
  const int nw = B.nw;
  const int ty0 = (int)blockIdx.x * kFillTile, tz0 = (int)blockIdx.y * kFillTile;
  for (int i = (int)threadIdx.x; i < kFillHalo * kFillHalo * nw; i += 256) {
    const int h = i / nw, w = i - h * nw;
    const int y = ty0 + h % kFillHalo - 1, z = tz0 + h / kFillHalo - 1;
    r[i] = (y >= 0 && y < B.ey && z >= 0 && z < B.ez) ? reach[((uint32_t)z * (uint32_t)B.ey + (uint32_t)y) * (uint32_t)nw + (uint32_t)w] : 0u;
  }
  for (int i = (int)threadIdx.x; i < kFillTile * kFillTile * nw; i += 256) {
    const int t = i / nw, w = i - t * nw;
    const int y = ty0 + t % kFillTile, z = tz0 + t / kFillTile;
    e[i] = (y < B.ey && z < B.ez) ? ~occ[((uint32_t)z * (uint32_t)B.ey + (uint32_t)y) * (uint32_t)nw + (uint32_t)w] & bitvol_valid(B, w) : 0u;
  }
  __syncthreads();
  int any = 0, changed;
  // Inside a round lanes read words of r[] that other lanes store in the same round, with no barrier between: deliberate.  A word
  // has one writer, a store only adds bits, and a 32-bit LDS access is whole, so a reader sees the word before or after the store,
  // both subsets of the fixed point; and whenever any lane stored, __syncthreads_or forces another round that sees it.
  do {
    changed = 0;
    for (int i = (int)threadIdx.x; i < kFillTile * kFillTile * nw; i += 256) {
      const uint32_t ee = e[i];
      if (!ee) continue;
      const int t = i / nw, w = i - t * nw;
      const int h = (t / kFillTile + 1) * kFillHalo + t % kFillTile + 1;
      const uint32_t old = r[h * nw + w];
      if (old == ee) continue;                               // all of it reached already
      uint32_t in = old;
      if (CONN == 6) {
        if (w > 0) in |= r[h * nw + w - 1] >> 31;
        if (w < nw - 1) in |= r[h * nw + w + 1] << 31;
        in |= r[(h - 1) * nw + w] | r[(h + 1) * nw + w] | r[(h - kFillHalo) * nw + w] | r[(h + kFillHalo) * nw + w];
      } else {
#pragma unroll
        for (int dz = -1; dz <= 1; dz++)
#pragma unroll
          for (int dy = -1; dy <= 1; dy++) in |= fill_spread(r, h + dz * kFillHalo + dy, w, nw);
      }
      const uint32_t now = fill_runs(ee, in & ee);
      if (now != old) { r[h * nw + w] = now; changed = 1; }
    }
    any |= changed;
  } while (__syncthreads_or(changed));
  if (any) {                                                 // a lane's words are the same in every round
    for (int i = (int)threadIdx.x; i < kFillTile * kFillTile * nw; i += 256) {
      const int t = i / nw, w = i - t * nw;
      const int y = ty0 + t % kFillTile, z = tz0 + t / kFillTile;
      if (y < B.ey && z < B.ez)
        reach[((uint32_t)z * (uint32_t)B.ey + (uint32_t)y) * (uint32_t)nw + (uint32_t)w] = r[((t / kFillTile + 1) * kFillHalo + t % kFillTile + 1) * nw + w];
    }
    *flag = 1u;
  }
}

// the enclosed bits of word g that the mask keeps
__device__ __forceinline__ uint32_t fill_enclosed_bits(const BitBox &B, const uint32_t *occ, const uint32_t *reach, uint32_t g,
                                                       const RegionShape *shapes, uint32_t n_shapes, int *x0, int *y, int *z) {
  const int w = bitvol_word(B, g, x0, y, z);
  const uint32_t bits = ~occ[g] & ~reach[g] & bitvol_valid(B, w);
  return n_shapes ? bitvol_inside(bits, shapes, n_shapes, *x0, *y, *z) : bits;
}

__global__ __launch_bounds__(256) void fill_count_kernel(const BitBox B, const uint32_t *occ, const uint32_t *reach, const RegionShape *shapes,
                                                        uint32_t n_shapes, uint32_t *count) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g > B.n_words) return;
  if (g == B.n_words) { count[g] = 0; return; }               // the scan's extra item: its slot receives the total
  int x0, y, z;
  count[g] = (uint32_t)__popc(fill_enclosed_bits(B, occ, reach, g, shapes, n_shapes, &x0, &y, &z));
}

// fixed: material + 1 of every enclosed voxel, or 0: inherit along -x from W (wkeys / wvals, n_w sorted pairs)
__global__ __launch_bounds__(256) void fill_emit_kernel(const BitBox B, const uint32_t *occ, const uint32_t *reach, const RegionShape *shapes,
                                                       uint32_t n_shapes, const uint32_t *excl, uint32_t fixed, const uint32_t *wkeys,
                                                       const uint32_t *wvals, uint32_t n_w, uint32_t *keys, uint32_t *vals) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= B.n_words || excl[g + 1u] == excl[g]) return;
  int x0, y, z;
  uint32_t pos = excl[g];
  for (uint32_t b = fill_enclosed_bits(B, occ, reach, g, shapes, n_shapes, &x0, &y, &z); b; b &= b - 1u) {
    const int bit = __ffs((int)b) - 1;
    uint32_t m = fixed;
    if (!m) {
      uint32_t below = occ[g] & ((1u << bit) - 1u);
      int xw = x0;
      for (uint32_t q = g; !below && xw > (B.wx0 << 5);) { q--; xw -= 32; below = occ[q]; }   // stays in the row: see the header
      m = below ? wvals[bitvol_find(wkeys, n_w, region_key(xw + 31 - __clz((int)below), y, z))] : 1u;
    }
    keys[pos] = region_key(x0 + bit, y, z); vals[pos] = m;
    pos++;
  }
}

namespace {

const char *kNoMemory = "out of device memory in the enclosed-space fill";

// what one call asks for, validated on the host before anything is queued
struct Request {
  tdt_fill f;
  std::vector<RegionShape> shapes;
};

int make_request(tdt_ctx *ctx, const tdt_fill *f, const tdt_region *regions, size_t n_regions, Request &R) {
  if (!f) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_fill pointer");
  if (f->connectivity != 6 && f->connectivity != 26) return fail(ctx, TDT_ERR_INVALID_VALUE, "connectivity must be 6 or 26");
  if (f->material < -1 || f->material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be -1 (inherit) or 0..253");
  R.f = *f;
  return region_shapes(ctx, regions, n_regions, &R.shapes);
}

// E(W, c) within the mask, or (with_walls) W + E(W, c), as {x, y, z, material + 1}, Morton-sorted, in device memory of ctx
// (allocated in S; null when *n == 0).  W: n_w voxels inside the grid of side 2^depth, Morton-sorted and unique, in device
// memory of ctx, n_w <= 2^26 (fill_list has checked the tree's list; a mesh's cannot be larger).  Queued on ctx's stream; synchronises.
int enclosed_voxels(tdt_ctx *front, tdt_ctx *ctx, const int4 *w, uint32_t n_w, int depth, const Request &R, bool with_walls, DeviceScratch &S,
                    const int4 **out, uint32_t *n) {
  *out = nullptr; *n = 0;
  front->fill_passes = 0;
  if (n_w == 0) return TDT_OK;                             // nothing encloses anything
  hipStream_t st = ctx->stream;
  // ---- bbox(W) ----
  int box[6];
  uint32_t *wk = S.get<uint32_t>(n_w), *wv = S.get<uint32_t>(n_w);
  if (!wk || !wv) return fail(front, TDT_ERR_HIP, kNoMemory);
  if (int rc = bitvol_list_bbox(front, st, w, n_w, depth, S, kNoMemory, "a wall voxel lies outside the grid", box)) return rc;
  BitBox B;
  bitvol_layout(box, box + 3, B);
  // ---- occupancy, seeds ----
  uint32_t *occ = S.get<uint32_t>(B.n_words), *reach = S.get<uint32_t>(B.n_words), *flags = S.get<uint32_t>(kBitvolBatch);
  if (!occ || !reach || !flags) return fail(front, TDT_ERR_HIP, kNoMemory);
  if (int rc = bitvol_rasterise(front, st, w, n_w, B, occ, wk, wv)) return rc;
  hipLaunchKernelGGL(fill_seed_kernel, dim3(blocks_of(B.n_words)), dim3(256), 0, st, B, (const uint32_t *)occ, reach);
  TDT_HIP(front, hipGetLastError());
  // ---- flood: a box thinner than 3 rows on an axis is all faces, and seeded whole ----
  if (B.ey > 2 && B.ez > 2 && B.hi[0] - B.lo[0] > 1) {
    const dim3 tiles((unsigned)((B.ey + kFillTile - 1) / kFillTile), (unsigned)((B.ez + kFillTile - 1) / kFillTile));
    auto flood = [&](uint32_t *flag) {
      if (R.f.connectivity == 6) hipLaunchKernelGGL(fill_flood_kernel<6>, tiles, dim3(256), 0, st, B, (const uint32_t *)occ, reach, flag);
      else hipLaunchKernelGGL(fill_flood_kernel<26>, tiles, dim3(256), 0, st, B, (const uint32_t *)occ, reach, flag);
    };
    if (int rc = bitvol_pass_loop(front, st, flags, flood, &front->fill_passes)) return rc;
  }
  // ---- count, emit, sort: W's own pairs in front for the solid forms; the cap is on the enclosed voxels alone ----
  RegionShape *d_shapes = nullptr;
  const uint32_t n_shapes = with_walls ? 0u : (uint32_t)R.shapes.size();
  if (int rc = upload_shapes(front, st, S, R.shapes.data(), n_shapes, kNoMemory, &d_shapes)) return rc;
  auto count = [&](uint32_t *cnt) {
    hipLaunchKernelGGL(fill_count_kernel, dim3(blocks_of((size_t)B.n_words + 1)), dim3(256), 0, st, B, (const uint32_t *)occ, (const uint32_t *)reach,
                       (const RegionShape *)d_shapes, n_shapes, cnt);
  };
  auto emit = [&](const uint32_t *excl, uint32_t *keys, uint32_t *vals) {
    hipLaunchKernelGGL(fill_emit_kernel, dim3(blocks_of(B.n_words)), dim3(256), 0, st, B, (const uint32_t *)occ, (const uint32_t *)reach,
                       (const RegionShape *)d_shapes, n_shapes, excl, R.f.material >= 0 ? (uint32_t)R.f.material + 1u : 0u, (const uint32_t *)wk,
                       (const uint32_t *)wv, n_w, keys, vals);
  };
  return bitvol_list_tail(front, st, B.n_words, count, emit, "the enclosed space", true, wk, wv, with_walls ? n_w : 0u, S, kNoMemory, out, n);
}

// the list a call produces on one single-device context: the tree form (mesh == null: E(V, c) within the mask) or the solid mesh
int fill_list(tdt_ctx *front, tdt_ctx *ctx, const Request &R, const tdt_mesh *mesh, int depth, DeviceScratch &S, const int4 **out, uint32_t *n) {
  if (mesh) {
    const int4 *s = nullptr;
    uint32_t ns = 0;
    if (int rc = mesh_voxels(front, ctx, mesh, depth, S, &s, &ns)) return rc;   // |S| <= its covered pairs <= 2^26, or it has failed
    return enclosed_voxels(front, ctx, s, ns, depth, R, true, S, out, n);
  }
  int4 *v = nullptr;
  uint32_t nv = 0;
  if (int rc = tree_voxels_capped(front, ctx, S, &v, &nv, &depth)) return rc;
  return enclosed_voxels(front, ctx, v, nv, depth, R, false, S, out, n);
}

struct FillSource final : VoxelSource {
  const Request &R;
  const tdt_mesh *mesh;
  FillSource(const Request &r, const tdt_mesh *m) : R(r), mesh(m) {}
  int run(tdt_ctx *front, tdt_ctx *ctx, int depth, DeviceScratch &S, const int4 **vox, uint32_t *n) override {
    return fill_list(front, ctx, R, mesh, depth, S, vox, n);
  }
};

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_extract_enclosed(tdt_ctx *ctx, const tdt_fill *f, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                                size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  Request R;
  if (int rc = make_request(ctx, f, regions, n_regions, R)) return rc;
  FillSource src(R, nullptr);
  return region_extract_source(ctx, src, 0, voxels_xyzm, capacity, n_voxels);
}

int tdt_octree_fill_enclosed(tdt_ctx *ctx, const tdt_fill *f, const tdt_region *regions, size_t n_regions, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  Request R;
  if (int rc = make_request(ctx, f, regions, n_regions, R)) return rc;
  FillSource src(R, nullptr);
  return region_edit_source(ctx, TDT_REGION_FILL, src, n_cells);
}

int tdt_voxelize_triangles_solid(tdt_ctx *ctx, const tdt_mesh *mesh, int depth, const tdt_fill *f, int32_t *voxels_xyzm, size_t capacity,
                                 size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  if (depth < 1 || depth > 10) return fail(ctx, TDT_ERR_INVALID_VALUE, "depth must be 1..10");
  if (int rc = check_mesh(ctx, mesh)) return rc;
  Request R;
  if (int rc = make_request(ctx, f, nullptr, 0, R)) return rc;
  FillSource src(R, mesh);
  return region_extract_source(ctx, src, depth, voxels_xyzm, capacity, n_voxels);
}

int tdt_octree_edit_triangles_solid(tdt_ctx *ctx, int op, const tdt_mesh *mesh, const tdt_fill *f, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (op < TDT_REGION_SET || op > TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  if (int rc = check_mesh(ctx, mesh)) return rc;
  Request R;
  if (int rc = make_request(ctx, f, nullptr, 0, R)) return rc;
  FillSource src(R, mesh);
  return region_edit_source(ctx, op, src, n_cells);
}

int tdt_debug_fill_passes(const tdt_ctx *ctx) { return ctx ? (int)ctx->fill_passes : 0; }

}  // extern "C"
