// Geodesic distance (include/tdt_rt.h tdt_octree_geodesic_field / tdt_octree_extract_geodesic / tdt_octree_edit_geodesic /
// tdt_octree_geodesic_path): g(q), the cheapest sum of step costs from any seed to q along paths that stay inside a medium P
// (the EMPTY voxels of the grid, or the tree's voxels, optionally of one material, optionally inside a mask), steps across a
// face / an edge / a corner costing w[0] / w[1] / w[2]; R = { g <= max_cost }.
//
// Like enclosed space this is a property of a dense neighbourhood, so the unit works on volumes over a box D of the grid (layout:
// bitvol_device.hpp; the steps between the tree's list and the volume: tdt_bitvol.hip).  D is the grid cut by whatever bounds
// R: the mask's bounding box, bbox(V) for the SOLID medium, and the seeds' bounding box grown by max_cost / (the smallest
// positive weight), since a step moves one voxel per axis at most and costs that much at least.
//
//   bbox, rasterise   tdt_bitvol.hip's: (SOLID) bbox(V), then V's occupancy bits over D and its (Morton key, material + 1).
//   medium     per word the bits of P: the occupancy (negated within the valid bits for EMPTY), a material match looked up in
//              V's sorted keys, the mask by the exact integer test of region edits per set bit.               geo_medium_kernel
//   seed       the cost volume, one 32-bit entry per PADDED voxel of D (a row is nw words = 32 nw entries, index = word * 32 +
//              bit): kGeoFar for a voxel of P, kGeoWall for every other one and for the padding, so the medium travels with the
//              cost and the relaxation needs no bit volume; then 0 for every seed that lies in P.  Both sentinels exceed
//              max_cost + 255 and their sum with a weight fits 32 unsigned bits.              geo_init_kernel, geo_seed_kernel
//   relax      one block of 256 lanes owns a tile of one word of x by 8 x 8 rows (32 x 8 x 8 voxels, aligned to the words in x
//              and to D's corner in y and z), held in LDS with a halo of one voxel all round (34 x 10 x 10 entries, 13.3 KiB;
//              the halo outside D is wall).  A lane owns one (x, y) and the 8 voxels along z.  A round computes, per voxel of P,
//                c = min(c, min(6 face neighbours) + w[0], min(12 edge neighbours) + w[1], min(8 corner neighbours) + w[2])
//              skipping a class whose weight is 0, and stores c only when it fell and is <= max_cost, which prunes the front.
//              A wall entry never changes and never passes the max_cost test as a source, so "both ends in P" needs no more.
//              Rounds repeat until __syncthreads_or reports no change (the lane's z order alternates, so a front runs through
//              the tile in either direction in one round); then the lanes that changed a value write their 8 back and raise
//              the pass's flag.  A tile whose halo'd block holds no finite value, or which owns no voxel of P, returns after
//              the load.                                                                                      geo_relax_kernel
//              tdt_fill.hip's argument carries over: values only fall, a tile has one writer, a 32-bit access is whole, so a
//              lane that reads a neighbour's entry (in LDS within a round, or in memory for its halo) sees an old or a new
//              value, both no smaller than the fixed point and both the cost of a real path; and a pass whose flag stays clear
//              changed nothing anywhere, so every block saw the final volume and found its tile stable: that is the fixed point,
//              which is g cut at max_cost.  The host queues the passes in batches with one flag read per batch
//              (bitvol_pass_loop).
//   reach      per padded voxel (cost < kGeoFar), a wave's ballot is two words of the reach volume.            geo_reach_kernel
//   count      per word popc of the reach bits; bitvol_list_tail scans them, reads the total, holds it to 2^26.  geo_count_kernel
//   emit       (Morton key, material + 1) per reached voxel at its word's offset, the material the fixed one or the voxel's own
//              by lookup in V's sorted keys; tdt_bitvol.hip's tail sorts the pairs and writes the list.         geo_emit_kernel
//   field      a gather over the requested box: the cost, or -1 outside D and where it is not finite.          geo_field_kernel
//   path       one wave walks back from the goal.  Lane l < 26 tests offset t = l (l < 13) or l + 1 in morphology's order
//              t = 9 (dx + 1) + 3 (dy + 1) + (dz + 1): inside D, finite, cost + w == the current cost; the lowest set lane of the
//              ballot is the canonical step.  At most g(goal) / w_min + 1 points.  It runs twice: to count, then into a buffer
//              of that size.                                                                                   geo_path_kernel
//   memory     per padded voxel of D (at most 2^27 unpadded): 4 B of cost, three bit volumes and a count per word (0.5 B);
//              besides V's list (16 B per voxel) and its pairs (8 B), and 32 B per resulting voxel.
#include <climits>
#include <string>
#include <vector>

#include "bitvol_device.hpp"
#include "device_scan.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr int kGeoTile = 8;                              // rows per tile side, in y and in z; a tile is one word wide in x
constexpr int kGeoHX = 34, kGeoHY = kGeoTile + 2, kGeoHZ = kGeoTile + 2;
constexpr int kGeoCells = kGeoHX * kGeoHY * kGeoHZ;      // 3400 entries
constexpr uint32_t kGeoFar = 0x7FFFFFFEu;                // in P, not reached
constexpr uint32_t kGeoWall = 0x7FFFFFFFu;               // not in P, or padding

struct GeoSteps {
  uint32_t w[3];               // face / edge / corner; 0: no such step
  uint32_t max_cost;
};

// the entry of voxel (x, y, z) of D in the cost volume
__device__ __forceinline__ uint32_t geo_index(const BitBox &B, int x, int y, int z) {
  return ((uint32_t)(z - B.lo[2]) * (uint32_t)B.ey + (uint32_t)(y - B.lo[1])) * ((uint32_t)B.nw * 32u) + (uint32_t)(x - (B.wx0 << 5));
}
__device__ __forceinline__ bool geo_in_box(const BitBox &B, int x, int y, int z) {
  return x >= B.lo[0] && x <= B.hi[0] && y >= B.lo[1] && y <= B.hi[1] && z >= B.lo[2] && z <= B.hi[2];
}
__device__ __forceinline__ uint32_t geo_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// solid: P inside V (match: material + 1 to keep, 0 any); otherwise P inside the empties.  masked: P inside the shapes' union
__global__ __launch_bounds__(256) void geo_medium_kernel(const BitBox B, const uint32_t *occ, int solid, uint32_t match, const uint32_t *wkeys,
                                                        const uint32_t *wvals, uint32_t n_w, const RegionShape *shapes, uint32_t n_shapes,
                                                        int masked, uint32_t *medium) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= B.n_words) return;
  int x0, y, z;
  const int w = bitvol_word(B, g, &x0, &y, &z);
  uint32_t bits = (solid ? occ[g] : ~occ[g]) & bitvol_valid(B, w);
  if (solid && match) {
    uint32_t kept = 0;
    for (uint32_t b = bits; b; b &= b - 1u) {
      const int bit = __ffs((int)b) - 1;
      if (wvals[bitvol_find(wkeys, n_w, region_key(x0 + bit, y, z))] == match) kept |= 1u << bit;
    }
    bits = kept;
  }
  if (masked) bits = bitvol_inside(bits, shapes, n_shapes, x0, y, z);
  medium[g] = bits;
}

__global__ __launch_bounds__(256) void geo_init_kernel(const BitBox B, const uint32_t *medium, uint32_t *cost) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= B.n_words * 32u) return;
  cost[i] = (medium[i >> 5] >> (i & 31u)) & 1u ? kGeoFar : kGeoWall;
}

// seeds: n triples inside the grid; one outside D or not in P is ignored
__global__ __launch_bounds__(256) void geo_seed_kernel(const BitBox B, const int32_t *seeds, uint32_t n, uint32_t *cost) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  const int x = seeds[3u * s], y = seeds[3u * s + 1u], z = seeds[3u * s + 2u];
  if (!geo_in_box(B, x, y, z)) return;
  const uint32_t at = geo_index(B, x, y, z);
  if (cost[at] != kGeoWall) cost[at] = 0u;
}

// grid: (words per row * tiles along y, tiles along z)
__global__ __launch_bounds__(256) void geo_relax_kernel(const BitBox B, uint32_t *cost, const GeoSteps W, uint32_t *flag) {
  __shared__ uint32_t c[kGeoCells];
  const int nw = B.nw, ex = nw * 32;
  const int w = (int)(blockIdx.x % (uint32_t)nw);
  const int ty0 = (int)(blockIdx.x / (uint32_t)nw) * kGeoTile, tz0 = (int)blockIdx.y * kGeoTile;
  int finite = 0, open = 0;
  for (int i = (int)threadIdx.x; i < kGeoCells; i += 256) {
    const int hx = i % kGeoHX, hy = (i / kGeoHX) % kGeoHY, hz = i / (kGeoHX * kGeoHY);
    const int xp = w * 32 + hx - 1, y = ty0 + hy - 1, z = tz0 + hz - 1;   // xp: the entry's place in its padded row
    uint32_t v = kGeoWall;
    if (xp >= 0 && xp < ex && y >= 0 && y < B.ey && z >= 0 && z < B.ez) v = cost[((uint32_t)z * (uint32_t)B.ey + (uint32_t)y) * (uint32_t)ex + (uint32_t)xp];
    c[i] = v;
    finite |= v < kGeoFar;
    open |= v != kGeoWall && hx >= 1 && hx <= 32 && hy >= 1 && hy <= kGeoTile && hz >= 1 && hz <= kGeoTile;
  }
  if (!__syncthreads_or(finite)) return;                     // nothing to spread from; (also the barrier behind the load)
  if (!__syncthreads_or(open)) return;                       // nothing to spread to
  const int lx = (int)(threadIdx.x & 31u), ly = (int)(threadIdx.x >> 5);
  const int base = kGeoHX * kGeoHY + (ly + 1) * kGeoHX + lx + 1;
  const int sy = kGeoHX, sz = kGeoHX * kGeoHY;
  int any = 0, changed, down = 0;
  // Inside a round lanes read entries of c[] that other lanes store in the same round, with no barrier between: deliberate, as
  // in tdt_fill.hip.  An entry has one writer, a store only lowers it to the cost of a real path, and a 32-bit LDS access is
  // whole; whenever any lane stored, __syncthreads_or forces another round that sees it.
  do {
    changed = 0;
    for (int k = 0; k < kGeoTile; k++) {
      const int at = base + (down ? kGeoTile - 1 - k : k) * sz;
      const uint32_t old = c[at];
      if (old == kGeoWall || old == 0u) continue;
      uint32_t m = geo_min(geo_min(geo_min(c[at - 1], c[at + 1]), geo_min(c[at - sy], c[at + sy])), geo_min(c[at - sz], c[at + sz]));
      uint32_t best = geo_min(old, m + W.w[0]);
      if (W.w[1]) {
        m = geo_min(geo_min(geo_min(c[at - sy - 1], c[at - sy + 1]), geo_min(c[at + sy - 1], c[at + sy + 1])),
                    geo_min(geo_min(c[at - sz - 1], c[at - sz + 1]), geo_min(c[at + sz - 1], c[at + sz + 1])));
        m = geo_min(m, geo_min(geo_min(c[at - sz - sy], c[at - sz + sy]), geo_min(c[at + sz - sy], c[at + sz + sy])));
        best = geo_min(best, m + W.w[1]);
      }
      if (W.w[2]) {
        m = geo_min(geo_min(geo_min(c[at - sz - sy - 1], c[at - sz - sy + 1]), geo_min(c[at - sz + sy - 1], c[at - sz + sy + 1])),
                    geo_min(geo_min(c[at + sz - sy - 1], c[at + sz - sy + 1]), geo_min(c[at + sz + sy - 1], c[at + sz + sy + 1])));
        best = geo_min(best, m + W.w[2]);
      }
      if (best < old && best <= W.max_cost) { c[at] = best; changed = 1; }
    }
    any |= changed;
    down ^= 1;
  } while (__syncthreads_or(changed));
  if (any) {                                                 // a lane's entries are the same in every round
    const int y = ty0 + ly;
    if (y < B.ey)
      for (int k = 0; k < kGeoTile; k++) {
        const int z = tz0 + k;
        if (z < B.ez) cost[((uint32_t)z * (uint32_t)B.ey + (uint32_t)y) * (uint32_t)ex + (uint32_t)(w * 32 + lx)] = c[base + k * sz];
      }
    *flag = 1u;
  }
}

__global__ __launch_bounds__(256) void geo_reach_kernel(const BitBox B, const uint32_t *cost, uint32_t *reach) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool live = i < B.n_words * 32u;
  const unsigned long long ballot = __ballot(live && cost[i] < kGeoFar);    // every lane of the block: no early return above
  if (live && (i & 31u) == 0u) reach[i >> 5] = (uint32_t)(ballot >> (threadIdx.x & 32u));
}

__global__ __launch_bounds__(256) void geo_count_kernel(const BitBox B, const uint32_t *reach, uint32_t *count) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g > B.n_words) return;
  count[g] = g == B.n_words ? 0u : (uint32_t)__popc(reach[g]);   // the scan's extra item: its slot receives the total
}

// fixed: material + 1 of every reached voxel, or 0: the voxel's own (SOLID: it is in V's n_w sorted pairs)
__global__ __launch_bounds__(256) void geo_emit_kernel(const BitBox B, const uint32_t *reach, const uint32_t *excl, uint32_t fixed,
                                                      const uint32_t *wkeys, const uint32_t *wvals, uint32_t n_w, uint32_t *keys, uint32_t *vals) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= B.n_words || excl[g + 1u] == excl[g]) return;
  int x0, y, z;
  bitvol_word(B, g, &x0, &y, &z);
  uint32_t pos = excl[g];
  for (uint32_t b = reach[g]; b; b &= b - 1u) {
    const int bit = __ffs((int)b) - 1;
    const uint32_t k = region_key(x0 + bit, y, z);
    keys[pos] = k; vals[pos] = fixed ? fixed : wvals[bitvol_find(wkeys, n_w, k)];
    pos++;
  }
}

// out over the inclusive box lo..hi, x fastest; have = 0: D is empty
__global__ __launch_bounds__(256) void geo_field_kernel(const BitBox B, const uint32_t *cost, int have, int lx, int ly, int lz, int ex, int ey,
                                                       uint32_t n, int32_t *out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int x = lx + (int)(i % (uint32_t)ex), y = ly + (int)((i / (uint32_t)ex) % (uint32_t)ey), z = lz + (int)(i / ((uint32_t)ex * (uint32_t)ey));
  int32_t v = -1;
  if (have && geo_in_box(B, x, y, z)) {
    const uint32_t cv = cost[geo_index(B, x, y, z)];
    if (cv < kGeoFar) v = (int32_t)cv;
  }
  out[i] = v;
}

// one wave.  result = {points, g(goal)} or {0, -1}; out (may be null): the first `capacity` points {x, y, z}
__global__ __launch_bounds__(64) void geo_path_kernel(const BitBox B, const uint32_t *cost, const GeoSteps W, uint32_t w_min, int have, int gx, int gy,
                                                     int gz, int32_t *out, uint32_t capacity, int32_t *result) {
  const int lane = (int)threadIdx.x;
  const int t = lane < 13 ? lane : lane + 1;
  const int dx = t / 9 - 1, dy = (t / 3) % 3 - 1, dz = t % 3 - 1;
  const uint32_t wk = lane < 26 ? W.w[(dx != 0) + (dy != 0) + (dz != 0) - 1] : 0u;
  uint32_t g = kGeoWall;
  if (have && geo_in_box(B, gx, gy, gz)) g = cost[geo_index(B, gx, gy, gz)];
  if (g >= kGeoFar) {                                        // the same in every lane
    if (lane == 0) { result[0] = 0; result[1] = -1; }
    return;
  }
  const uint32_t total = g, bound = g / w_min + 1u;
  int x = gx, y = gy, z = gz;
  uint32_t n = 0;
  for (;;) {
    if (lane == 0 && out && n < capacity) { out[3u * n] = x; out[3u * n + 1u] = y; out[3u * n + 2u] = z; }
    n++;
    if (g == 0u || n >= bound) break;
    const int qx = x + dx, qy = y + dy, qz = z + dz;
    bool ok = false;
    if (wk && geo_in_box(B, qx, qy, qz)) {
      const uint32_t cq = cost[geo_index(B, qx, qy, qz)];
      ok = cq < kGeoFar && cq + wk == g;
    }
    const uint32_t pick = (uint32_t)__ballot(ok);            // lanes 0..25: the low word
    if (!pick) break;                                        // (a fixed point always has a predecessor)
    const int l = __ffs((int)pick) - 1, tt = l < 13 ? l : l + 1;
    const int ux = tt / 9 - 1, uy = (tt / 3) % 3 - 1, uz = tt % 3 - 1;
    x += ux; y += uy; z += uz;
    g -= W.w[(ux != 0) + (uy != 0) + (uz != 0) - 1];
  }
  if (lane == 0) { result[0] = (int32_t)n; result[1] = (int32_t)total; }
}

namespace {

const char *kNoMemory = "out of device memory in the geodesic distance";

// what one call asks for, validated on the host before anything is queued
struct Request {
  tdt_geodesic g;
  bool masked = false;
  std::vector<RegionShape> shapes;
  std::vector<int32_t> seeds;    // triples, as given
};

int make_request(tdt_ctx *ctx, const tdt_geodesic *g, bool list_form, const int32_t *seeds, size_t n_seeds, const tdt_region *regions,
                 size_t n_regions, Request &R) {
  if (!g) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_geodesic pointer");
  if (g->medium != TDT_MEDIUM_EMPTY && g->medium != TDT_MEDIUM_SOLID) return fail(ctx, TDT_ERR_INVALID_VALUE, "medium must be a TDT_MEDIUM_* value");
  if (g->match < -1 || g->match > 253 || (g->medium == TDT_MEDIUM_EMPTY && g->match != -1))
    return fail(ctx, TDT_ERR_INVALID_VALUE, "match must be -1 or, in the SOLID medium, 0..253");
  if (g->w[0] < 1 || g->w[0] > 255) return fail(ctx, TDT_ERR_INVALID_VALUE, "w[0] must be 1..255");
  if (g->w[1] < 0 || g->w[1] > 255 || g->w[2] < 0 || g->w[2] > 255) return fail(ctx, TDT_ERR_INVALID_VALUE, "w[1] and w[2] must be 0..255");
  if (g->max_cost < 0 || g->max_cost > (1 << 30)) return fail(ctx, TDT_ERR_INVALID_VALUE, "max_cost must be 0..2^30");
  if (g->material < -1 || g->material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be -1 (the voxel's own) or 0..253");
  if (list_form && g->medium == TDT_MEDIUM_EMPTY && g->material < 0)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "an EMPTY voxel has no material of its own: material must be 0..253");
  if (g->pad != 0) return fail(ctx, TDT_ERR_INVALID_VALUE, "pad must be 0");
  if (n_seeds && !seeds) return fail(ctx, TDT_ERR_INVALID_VALUE, "null seed list");
  if (n_seeds >= (1ull << 31) / 3) return fail(ctx, TDT_ERR_INVALID_VALUE, "too many seeds");
  R.g = *g;
  R.masked = n_regions > 0;
  if (int rc = region_shapes(ctx, regions, n_regions, &R.shapes)) return rc;
  R.seeds.assign(seeds, seeds + 3 * n_seeds);
  return TDT_OK;
}

inline uint32_t smallest_weight(const tdt_geodesic &g) {
  int m = g.w[0];
  if (g.w[1] > 0 && g.w[1] < m) m = g.w[1];
  if (g.w[2] > 0 && g.w[2] < m) m = g.w[2];
  return (uint32_t)m;
}

// The part of D the host knows without the tree: the grid cut by the mask's bounding box and by the in-grid seeds' bounding box
// grown by max_cost / w_min; seeds_in: those seeds.  false: it is empty.
bool host_domain(const Request &R, int depth, long long lo[3], long long hi[3], std::vector<int32_t> &seeds_in) {
  const long long N = 1ll << depth;
  for (int a = 0; a < 3; a++) { lo[a] = 0; hi[a] = N - 1; }
  if (R.masked) {
    long long mlo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, mhi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
    for (const RegionShape &s : R.shapes)
      for (int a = 0; a < 3; a++) {
        const long long l = s.shape == TDT_SHAPE_BOX ? (long long)s.a[a] : (long long)s.a[a] - s.b[0];
        const long long h = s.shape == TDT_SHAPE_BOX ? (long long)s.b[a] : (long long)s.a[a] + s.b[0];
        if (s.shape == TDT_SHAPE_BOX && (s.a[0] > s.b[0] || s.a[1] > s.b[1] || s.a[2] > s.b[2])) continue;   // an empty box
        mlo[a] = l < mlo[a] ? l : mlo[a]; mhi[a] = h > mhi[a] ? h : mhi[a];
      }
    for (int a = 0; a < 3; a++) { lo[a] = mlo[a] > lo[a] ? mlo[a] : lo[a]; hi[a] = mhi[a] < hi[a] ? mhi[a] : hi[a]; }
  }
  long long slo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, shi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
  seeds_in.clear();
  for (size_t s = 0; s + 2 < R.seeds.size(); s += 3) {
    const int32_t *p = &R.seeds[s];
    if (p[0] < 0 || p[0] >= N || p[1] < 0 || p[1] >= N || p[2] < 0 || p[2] >= N) continue;
    seeds_in.insert(seeds_in.end(), p, p + 3);
    for (int a = 0; a < 3; a++) { slo[a] = p[a] < slo[a] ? p[a] : slo[a]; shi[a] = p[a] > shi[a] ? p[a] : shi[a]; }
  }
  if (seeds_in.empty()) return false;
  const long long grow = (long long)R.g.max_cost / (long long)smallest_weight(R.g);
  for (int a = 0; a < 3; a++) {
    lo[a] = slo[a] - grow > lo[a] ? slo[a] - grow : lo[a];
    hi[a] = shi[a] + grow < hi[a] ? shi[a] + grow : hi[a];
    if (lo[a] > hi[a]) return false;
  }
  return true;
}

int check_cap(tdt_ctx *front, const long long lo[3], const long long hi[3]) {
  unsigned long long voxels = 1;
  for (int a = 0; a < 3; a++) voxels *= (unsigned long long)(hi[a] - lo[a] + 1);
  if (voxels > TDT_GEODESIC_DOMAIN_CAP)
    return fail(front, TDT_ERR_INVALID_VALUE, "the geodesic domain holds " + std::to_string(voxels) + " voxels (more than 2^27)");
  return TDT_OK;
}

// the relaxed cost volume of one call, in S
struct Solved {
  bool have = false;             // false: D is empty, so is R
  BitBox B;
  uint32_t *cost = nullptr, *wk = nullptr, *wv = nullptr;
  uint32_t nv = 0;
  GeoSteps W;
};

// g over D on one single-device context.  Queued on ctx's stream; synchronises (the tree walk, SOLID's bounding box, once per
// batch of passes).  depth_known: the max_depth of slot 7 when the caller has it already (> 0), for the early domain check.
int solve(tdt_ctx *front, tdt_ctx *ctx, const Request &R, int depth_known, DeviceScratch &S, Solved &Z) {
  const tdt_geodesic &Q = R.g;
  const bool solid = Q.medium == TDT_MEDIUM_SOLID;
  front->geodesic_passes = 0;
  Z.have = false;
  for (int k = 0; k < 3; k++) Z.W.w[k] = (uint32_t)Q.w[k];
  Z.W.max_cost = (uint32_t)Q.max_cost;
  long long lo[3], hi[3];
  std::vector<int32_t> seeds_in;
  // the EMPTY medium's domain is known without the tree: its cap is checked before the tree is walked
  if (!solid && depth_known > 0 && host_domain(R, depth_known, lo, hi, seeds_in))
    if (int rc = check_cap(front, lo, hi)) return rc;
  hipStream_t st = ctx->stream;
  int4 *v = nullptr;
  uint32_t nv = 0;
  int depth = 0;
  if (int rc = tree_voxels_capped(front, ctx, S, &v, &nv, &depth)) return rc;
  if (!host_domain(R, depth, lo, hi, seeds_in)) return TDT_OK;
  if (solid) {
    if (nv == 0) return TDT_OK;
    int box[6];
    if (int rc = bitvol_list_bbox(front, st, v, nv, depth, S, kNoMemory, "a voxel lies outside the grid", box)) return rc;
    for (int a = 0; a < 3; a++) {
      lo[a] = box[a] > lo[a] ? box[a] : lo[a];
      hi[a] = box[3 + a] < hi[a] ? box[3 + a] : hi[a];
      if (lo[a] > hi[a]) return TDT_OK;
    }
  }
  if (int rc = check_cap(front, lo, hi)) return rc;
  const int ilo[3] = {(int)lo[0], (int)lo[1], (int)lo[2]}, ihi[3] = {(int)hi[0], (int)hi[1], (int)hi[2]};
  BitBox &B = Z.B;
  bitvol_layout(ilo, ihi, B);
  // ---- volumes ----
  const size_t padded = (size_t)B.n_words * 32;            // < 2^28: the cap, and at most 62 voxels of padding per row
  uint32_t *occ = S.get<uint32_t>(B.n_words), *medium = S.get<uint32_t>(B.n_words), *flags = S.get<uint32_t>(kBitvolBatch);
  uint32_t *cost = S.get<uint32_t>(padded);
  Z.wk = S.get<uint32_t>(nv); Z.wv = S.get<uint32_t>(nv);
  int32_t *d_seeds = S.get<int32_t>(seeds_in.size());
  if (!occ || !medium || !flags || !cost || !Z.wk || !Z.wv || !d_seeds) return fail(front, TDT_ERR_HIP, kNoMemory);
  RegionShape *d_shapes = nullptr;
  const uint32_t n_shapes = (uint32_t)R.shapes.size();
  if (int rc = upload_shapes(front, st, S, R.shapes.data(), n_shapes, kNoMemory, &d_shapes)) return rc;
  TDT_HIP(front, hipMemcpyAsync(d_seeds, seeds_in.data(), seeds_in.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (int rc = bitvol_rasterise(front, st, v, nv, B, occ, Z.wk, Z.wv)) return rc;
  // ---- medium, seeds ----
  const uint32_t n_seeds = (uint32_t)(seeds_in.size() / 3);
  hipLaunchKernelGGL(geo_medium_kernel, dim3(blocks_of(B.n_words)), dim3(256), 0, st, B, (const uint32_t *)occ, solid ? 1 : 0,
                     Q.match >= 0 ? (uint32_t)Q.match + 1u : 0u, (const uint32_t *)Z.wk, (const uint32_t *)Z.wv, nv, (const RegionShape *)d_shapes, n_shapes,
                     R.masked ? 1 : 0, medium);
  hipLaunchKernelGGL(geo_init_kernel, dim3(blocks_of(padded)), dim3(256), 0, st, B, (const uint32_t *)medium, cost);
  hipLaunchKernelGGL(geo_seed_kernel, dim3(blocks_of(n_seeds)), dim3(256), 0, st, B, (const int32_t *)d_seeds, n_seeds, cost);
  TDT_HIP(front, hipGetLastError());
  // ---- relax ----
  const dim3 tiles((unsigned)B.nw * (unsigned)((B.ey + kGeoTile - 1) / kGeoTile), (unsigned)((B.ez + kGeoTile - 1) / kGeoTile));
  auto relax = [&](uint32_t *flag) { hipLaunchKernelGGL(geo_relax_kernel, tiles, dim3(256), 0, st, B, cost, Z.W, flag); };
  if (int rc = bitvol_pass_loop(front, st, flags, relax, &front->geodesic_passes)) return rc;
  Z.cost = cost; Z.nv = nv; Z.have = true;
  return TDT_OK;
}

// R as {x, y, z, material + 1}, Morton-sorted, in device memory of ctx (allocated in S; null when *n == 0)
int geodesic_list(tdt_ctx *front, tdt_ctx *ctx, const Request &R, int depth_known, DeviceScratch &S, const int4 **out, uint32_t *n) {
  *out = nullptr; *n = 0;
  Solved Z;
  if (int rc = solve(front, ctx, R, depth_known, S, Z)) return rc;
  if (!Z.have) return TDT_OK;
  hipStream_t st = ctx->stream;
  const BitBox &B = Z.B;
  uint32_t *reach = S.get<uint32_t>(B.n_words);
  if (!reach) return fail(front, TDT_ERR_HIP, kNoMemory);
  auto count = [&](uint32_t *cnt) {
    hipLaunchKernelGGL(geo_reach_kernel, dim3(blocks_of((unsigned long long)B.n_words * 32u)), dim3(256), 0, st, B, (const uint32_t *)Z.cost, reach);
    hipLaunchKernelGGL(geo_count_kernel, dim3(blocks_of((size_t)B.n_words + 1)), dim3(256), 0, st, B, (const uint32_t *)reach, cnt);
  };
  auto emit = [&](const uint32_t *excl, uint32_t *keys, uint32_t *vals) {
    hipLaunchKernelGGL(geo_emit_kernel, dim3(blocks_of(B.n_words)), dim3(256), 0, st, B, (const uint32_t *)reach, excl,
                       R.g.material >= 0 ? (uint32_t)R.g.material + 1u : 0u, (const uint32_t *)Z.wk, (const uint32_t *)Z.wv, Z.nv, keys, vals);
  };
  return bitvol_list_tail(front, st, B.n_words, count, emit, "the reach set", true, nullptr, nullptr, 0u, S, kNoMemory, out, n);
}

struct GeodesicSource final : VoxelSource {
  const Request &R;
  explicit GeodesicSource(const Request &r) : R(r) {}
  int run(tdt_ctx *front, tdt_ctx *ctx, int depth, DeviceScratch &S, const int4 **vox, uint32_t *n) override {
    return geodesic_list(front, ctx, R, depth, S, vox, n);
  }
};

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_geodesic_field(tdt_ctx *ctx, const tdt_geodesic *g, const int32_t *seeds_xyz, size_t n_seeds, const tdt_region *regions,
                              size_t n_regions, const int32_t lo[3], const int32_t hi[3], int32_t *field, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  if (!lo || !hi) return fail(ctx, TDT_ERR_INVALID_VALUE, "null box pointer");
  Request R;
  if (int rc = make_request(ctx, g, false, seeds_xyz, n_seeds, regions, n_regions, R)) return rc;
  tdt_ctx *m = first_member(ctx);
  // everything the host can check comes first: the count-only call walks no tree and queues nothing
  int depth = 0;
  if (int rc = walk_inputs(ctx, m, &depth)) return rc;
  if (int rc = bitvol_field_box(ctx, depth, lo, hi, [] { return TDT_OK; }, field != nullptr, capacity, n_voxels)) return rc;
  if (!field) return TDT_OK;
  const size_t count = *n_voxels;
  TDT_HIP(ctx, hipSetDevice(m->device));
  hipStream_t st = m->stream;
  Drain drain{st};
  DeviceScratch S;
  Solved Z;
  if (int rc = solve(ctx, m, R, depth, S, Z)) { *n_voxels = 0; return rc; }
  int32_t *d_field = S.get<int32_t>((size_t)count);
  if (!d_field) { *n_voxels = 0; return fail(ctx, TDT_ERR_HIP, kNoMemory); }
  if (!Z.have) { const int z3[3] = {0, 0, 0}; bitvol_layout(z3, z3, Z.B); }
  hipLaunchKernelGGL(geo_field_kernel, dim3(blocks_of(count)), dim3(256), 0, st, Z.B, (const uint32_t *)Z.cost, Z.have ? 1 : 0, (int)lo[0], (int)lo[1],
                     (int)lo[2], (int)(hi[0] - lo[0] + 1), (int)(hi[1] - lo[1] + 1), (uint32_t)count, d_field);
  TDT_HIP(ctx, hipGetLastError());
  TDT_HIP(ctx, hipMemcpyAsync(field, d_field, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  TDT_HIP(ctx, hipStreamSynchronize(st));
  return TDT_OK;
}

int tdt_octree_extract_geodesic(tdt_ctx *ctx, const tdt_geodesic *g, const int32_t *seeds_xyz, size_t n_seeds, const tdt_region *regions,
                                size_t n_regions, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  Request R;
  if (int rc = make_request(ctx, g, true, seeds_xyz, n_seeds, regions, n_regions, R)) return rc;
  tdt_ctx *m = first_member(ctx);
  int depth = 0;
  if (int rc = walk_inputs(ctx, m, &depth)) return rc;
  GeodesicSource src(R);
  return region_extract_source(ctx, src, depth, voxels_xyzm, capacity, n_voxels);
}

int tdt_octree_edit_geodesic(tdt_ctx *ctx, int op, const tdt_geodesic *g, const int32_t *seeds_xyz, size_t n_seeds, const tdt_region *regions,
                             size_t n_regions, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  Request R;
  if (int rc = make_request(ctx, g, true, seeds_xyz, n_seeds, regions, n_regions, R)) return rc;
  if (op < TDT_REGION_SET || op > TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  GeodesicSource src(R);
  return region_edit_source(ctx, op, src, n_cells);
}

int tdt_octree_geodesic_path(tdt_ctx *ctx, const tdt_geodesic *g, const int32_t *seeds_xyz, size_t n_seeds, const tdt_region *regions,
                             size_t n_regions, const int32_t goal[3], int32_t *path_xyz, size_t capacity, size_t *n_points, int32_t *cost) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_points || !cost) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_points or cost pointer");
  *n_points = 0; *cost = -1;
  if (!goal) return fail(ctx, TDT_ERR_INVALID_VALUE, "null goal pointer");
  Request R;
  if (int rc = make_request(ctx, g, false, seeds_xyz, n_seeds, regions, n_regions, R)) return rc;
  tdt_ctx *m = first_member(ctx);
  int depth = 0;
  if (int rc = walk_inputs(ctx, m, &depth)) return rc;
  TDT_HIP(ctx, hipSetDevice(m->device));
  hipStream_t st = m->stream;
  Drain drain{st};
  DeviceScratch S;
  Solved Z;
  if (int rc = solve(ctx, m, R, depth, S, Z)) return rc;
  if (!Z.have) return TDT_OK;                              // R is empty: the goal is not in it
  int32_t *d_result = S.get<int32_t>(2), h_result[2] = {0, -1};
  if (!d_result) return fail(ctx, TDT_ERR_HIP, kNoMemory);
  const uint32_t w_min = smallest_weight(R.g);
  hipLaunchKernelGGL(geo_path_kernel, dim3(1), dim3(64), 0, st, Z.B, (const uint32_t *)Z.cost, Z.W, w_min, 1, (int)goal[0], (int)goal[1], (int)goal[2],
                     (int32_t *)nullptr, 0u, d_result);
  TDT_HIP(ctx, hipGetLastError());
  TDT_HIP(ctx, hipMemcpyAsync(h_result, d_result, sizeof h_result, hipMemcpyDeviceToHost, st));
  TDT_HIP(ctx, hipStreamSynchronize(st));                  // the count
  const size_t n = (size_t)h_result[0];
  *n_points = n; *cost = h_result[1];
  if (!path_xyz || n == 0) return TDT_OK;
  if (capacity < n) return fail(ctx, TDT_ERR_INVALID_VALUE, "capacity " + std::to_string(capacity) + " < " + std::to_string(n) + " points");
  int32_t *d_path = S.get<int32_t>(3 * n);
  if (!d_path) return fail(ctx, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(geo_path_kernel, dim3(1), dim3(64), 0, st, Z.B, (const uint32_t *)Z.cost, Z.W, w_min, 1, (int)goal[0], (int)goal[1], (int)goal[2],
                     d_path, (uint32_t)n, d_result);
  TDT_HIP(ctx, hipGetLastError());
  TDT_HIP(ctx, hipMemcpyAsync(path_xyz, d_path, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  TDT_HIP(ctx, hipStreamSynchronize(st));
  return TDT_OK;
}

int tdt_debug_geodesic_passes(const tdt_ctx *ctx) { return ctx ? (int)ctx->geodesic_passes : 0; }

}  // extern "C"
