// Exact Euclidean distance (include/tdt_rt.h tdt_octree_morph_round / tdt_octree_extract_morph_round / tdt_octree_distance_field):
// the squared distance d2(q, S) of every voxel of a domain box to the nearest voxel of a set S, with that voxel, by a separable
// transform of three passes whatever the radius (margin, halo and scan length grow with R); thresholded it is the round grow / shrink / open / close / hollow.
//
// The domain is bbox(V) (round ops) or the requested box (field) grown by R = ceil(sqrt(radius2)) and clipped to the grid; it is
// laid out as bitvol_device.hpp describes (the layout enclosed space uses too): x along 32-bit words, rows word-aligned in
// ABSOLUTE x, so a row is nw words = 32 nw padded voxels, and the byte volumes below use the same padded rows
// (index = row * 32 nw + x - 32 wx0).
//
//   bbox, rasterise   tdt_bitvol.hip's: (round ops) bbox(V), then the occupancy bits of the voxels of V inside the domain and every
//              voxel's (Morton key, material + 1) for the material lookups.
//   pass x     one lane per padded voxel: the nearest set bit of its row within +-R from a count of leading / trailing zeros
//              over its word and at most two words either side; of two at the same distance the lower x.  One signed byte
//              per voxel, -128 = none within R.                                                          dist_pass_x_kernel
//   pass y, z  one kernel, dist_scan_kernel<MODE>.  A block of 4 waves owns 64 x of 64 rows along the scanned axis at one
//              index of the other axis, and stages those rows with a halo of R either side in LDS as 16-bit pairs of offset
//              bytes ((64 + 2 R) x 64 x 2 B <= 24 KiB).  A lane is one x; a wave's 64 lanes read 64 consecutive 16-bit
//              values of a row, 32 banks once each.  Each lane walks outward from offset 0 and stops when offset^2 exceeds
//              its best sum.  The candidates are compared as ONE 64-bit key (sum << 32 | x offset | y offset | this offset),
//              so among equal sums the lexicographically lowest (x, y, z) wins whatever the scan order.  Sums above R^2 are
//              dropped: they cannot be part of a result <= R^2.
//              pass y writes the pair (x offset, y offset) per voxel.  pass z writes no offset volume but feeds its consumer:
//                bits   the wave's ballot of (d2 <= radius2) is two words of a bit volume, optionally complemented and ANDed
//                       with another volume, which turns the five ops into one or two transforms (see round_list);
//                       with an inherited material it also keeps the z offset of the nearest voxel, one byte: the pair
//                       stored at (x, y, z + that offset) is the rest of it, so CLOSE still finds D's nearest voxel after its
//                       second transform.  (A deviation from "no third volume": the alternative is to run pass z a third
//                       time at the emit.)
//                field  the signed, clamped squared distance and the nearest voxel, straight into the result arrays.
//   The complement (the erode side): the source bits are inverted as they are read, every in-grid voxel outside the domain
//   is empty and so a candidate at offset 0 (words beyond the row in pass x, halo rows beyond the domain in the scans), and
//   with border 0 the nearest lattice point outside the grid lies straight along an axis, at min over axes of
//   min(p + 1, N - p): the consumer takes the minimum with its square.
//   count, emit  per word popc of the selected bits — the result's difference from V inside the mask (the edit forms: a FILL or
//              CLEAR list for region_edit_source) or V with that difference applied (the extract forms) — exclusive_scan_u32,
//              then (Morton key, material + 1) per voxel: V's material by lookup in its sorted keys, a new voxel's the fixed
//              one or its nearest voxel's.  tdt_bitvol.hip's tail writes the list, sorting the extract forms first.
//                                                                                       dist_count_kernel, dist_emit_kernel
//   synchronisations per call: the tree walk, the bounding box, the count, the end; none depends on the radius.
//   memory     per PADDED domain voxel (rows rounded out to whole words; at most 2^28 unpadded): 1 B (pass x) + 2 B (pass
//              y), + 1 B + 2 B for an inherited DILATE / CLOSE, + 3 bit volumes and a count per word: at most 6.5 B.
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "bitvol_device.hpp"
#include "device_scan.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr int kDistTile = 64;                          // rows along the scanned axis per block
constexpr int kDistMaxR = 64;
constexpr int kDistRows = kDistTile + 2 * kDistMaxR;
constexpr int kDistNone = -128;                        // pass x: nothing within R
constexpr unsigned kDistSelf = (128u << 8) | 128u;     // the pair of offsets (0, 0); a pair of 0 = none

struct DistBox : BitBox {      // the domain and the layout of the volumes over it
  int32_t N, R;                // grid side; window
};

struct DistOut {               // what pass z does with a voxel's squared distance
  uint32_t *bits;              // bits: the result volume
  const uint32_t *andv;        // ANDed into it (null: the domain's valid bits)
  signed char *oz;             // the z offset of the nearest voxel (null: not kept)
  int32_t neg, r2;             // complement before the AND; the threshold
  int32_t edge;                // 1: the points outside the grid count as set (the erode side with border 0)
  int32_t *field, *nearest;    // field: the result arrays over the box blo..bhi (nearest may be null)
  int32_t blo[3], bhi[3];
  int32_t max_d2;
};

// the bits of word w (any integer, also beyond the row) whose x lies inside the grid
__device__ __forceinline__ uint32_t dist_grid(const DistBox &B, int w) {
  const int x0 = (B.wx0 + w) * 32;
  if (x0 < 0 || x0 >= B.N) return 0u;
  const int left = B.N - x0;
  return left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
}

// word w of a row of the source, or of its complement within the grid
__device__ __forceinline__ uint32_t dist_word(const DistBox &B, const uint32_t *src, uint32_t row, int w, int invert) {
  const uint32_t v = (w >= 0 && w < B.nw) ? src[row * (uint32_t)B.nw + (uint32_t)w] : 0u;
  return invert ? ~v & dist_grid(B, w) : v;
}

__global__ __launch_bounds__(256) void dist_pass_x_kernel(const DistBox B, const uint32_t *src, int invert, signed char *ox) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= B.n_words * 32u) return;
  const uint32_t wg = g >> 5;
  const int b = (int)(g & 31u), w = (int)(wg % (uint32_t)B.nw);
  const uint32_t row = wg / (uint32_t)B.nw;
  const int kw = (B.R + 31) >> 5;                            // words either side that can hold a bit within R
  const uint32_t c = dist_word(B, src, row, w, invert);
  int dl = INT_MAX, dh = INT_MAX;
  uint32_t m = c & (0xFFFFFFFFu >> (31 - b));                // x' <= x
  if (m) dl = b - (31 - __clz((int)m));
  else
    for (int k = 1; k <= kw; k++) {
      m = dist_word(B, src, row, w - k, invert);
      if (m) { dl = b + 32 * k - (31 - __clz((int)m)); break; }
    }
  m = c & (0xFFFFFFFEu << b);                                // x' > x
  if (m) dh = __ffs((int)m) - 1 - b;
  else
    for (int k = 1; k <= kw; k++) {
      m = dist_word(B, src, row, w + k, invert);
      if (m) { dh = 32 * k + __ffs((int)m) - 1 - b; break; }
    }
  int o = kDistNone;
  if (dl <= dh) { if (dl <= B.R) o = -dl; }                  // a tie: the lower x
  else if (dh <= B.R) o = dh;
  ox[g] = (signed char)o;
}

// one candidate of a lane's scan: c = the pair stored at signed offset dd along the scanned axis
__device__ __forceinline__ void dist_consider(unsigned c, int dd, unsigned long long &best) {
  if (!(c & 0xFFu)) return;
  const int ox = (int)(c & 0xFFu) - 128, oy = (int)(c >> 8) - 128;
  const unsigned sum = (unsigned)(ox * ox + oy * oy + dd * dd);
  const unsigned long long key = ((unsigned long long)sum << 32) | ((unsigned long long)(c & 0xFFu) << 16) | ((c >> 8) << 8) | (unsigned)(dd + 128);
  if (key < best) best = key;
}

// MODE 0: pass y (ox -> xy_out).  MODE 1: pass z, bits.  MODE 2: pass z, field.  grid: (64-wide x tiles, tiles along the
// scanned axis * the extent of the other axis)
template <int MODE>
__global__ __launch_bounds__(256) void dist_scan_kernel(const DistBox B, int invert, const signed char *ox, const unsigned short *xy_in,
                                                       unsigned short *xy_out, const DistOut O) {
  __shared__ unsigned short s[kDistRows * 64];
  const int R = B.R, ex = B.nw * 32;
  const int lx = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
  const int xi = (int)blockIdx.x * 64 + lx;                  // x within the padded row
  const int ea = MODE == 0 ? B.ey : B.ez;                    // extent of the scanned axis
  const int tiles = (ea + kDistTile - 1) / kDistTile;
  const int a0 = ((int)blockIdx.y % tiles) * kDistTile, other = (int)blockIdx.y / tiles;
  const int own = ea - a0 < kDistTile ? ea - a0 : kDistTile; // rows of this tile
  const int alo = B.lo[MODE == 0 ? 1 : 2];
  for (int i = (int)threadIdx.x; i < (own + 2 * R) * 64; i += 256) {
    const int a = a0 - R + (i >> 6), xl = (int)blockIdx.x * 64 + (i & 63);
    unsigned c = 0;
    if (xl < ex) {
      if (a >= 0 && a < ea) {
        const uint32_t row = MODE == 0 ? (uint32_t)other * (uint32_t)B.ey + (uint32_t)a : (uint32_t)a * (uint32_t)B.ey + (uint32_t)other;
        const uint32_t idx = row * (uint32_t)ex + (uint32_t)xl;
        if (MODE == 0) { const int o = ox[idx]; c = o == kDistNone ? 0u : (128u << 8) | (unsigned)(o + 128); }
        else c = xy_in[idx];
      } else if (invert && alo + a >= 0 && alo + a < B.N && B.wx0 * 32 + xl < B.N) {
        c = kDistSelf;                                       // beyond the domain, inside the grid: empty
      }
    }
    s[i] = (unsigned short)c;
  }
  __syncthreads();
  const unsigned long long none = (unsigned long long)(R * R + 1) << 32;
  for (int k = 0; k < kDistTile / 4; k++) {                  // the same trip count in every wave: the ballot below
    const int r = wv + 4 * k, a = a0 + r;
    const bool live = r < own && xi < ex;
    unsigned long long best = none;
    if (live) {
      for (int d = 0; d <= R; d++) {
        if ((unsigned)(d * d) > (unsigned)(best >> 32)) break;
        dist_consider(s[(r + R - d) * 64 + lx], -d, best);
        if (d) dist_consider(s[(r + R + d) * 64 + lx], d, best);
      }
    }
    const bool found = best < none;
    const int sum = (int)(best >> 32);
    const int oa = (int)(best & 0xFFu) - 128;                // the offset along the scanned axis
    const uint32_t row = MODE == 0 ? (uint32_t)other * (uint32_t)B.ey + (uint32_t)a : (uint32_t)a * (uint32_t)B.ey + (uint32_t)other;
    const uint32_t idx = row * (uint32_t)ex + (uint32_t)xi;
    const int x = B.wx0 * 32 + xi, y = B.lo[1] + (MODE == 0 ? a : other), z = B.lo[2] + (MODE == 0 ? other : a);
    int e2 = INT_MAX;                                        // the squared distance to the outside of the grid
    if (MODE != 0 && O.edge) {
      int e = x + 1 < B.N - x ? x + 1 : B.N - x;
      e = y + 1 < e ? y + 1 : e; e = B.N - y < e ? B.N - y : e;
      e = z + 1 < e ? z + 1 : e; e = B.N - z < e ? B.N - z : e;
      e2 = e * e;
    }
    if (MODE == 0) {
      if (live) xy_out[idx] = found ? (unsigned short)(((unsigned)(oa + 128) << 8) | (unsigned)((best >> 16) & 0xFFu)) : (unsigned short)0;
    } else if (MODE == 1) {
      const bool within = live && ((found && sum <= O.r2) || e2 <= O.r2);
      const unsigned long long ballot = __ballot(within);
      if (r < own && (lx & 31) == 0) {
        const int w = (int)blockIdx.x * 2 + (lx >> 5);
        if (w < B.nw) {
          const uint32_t g = row * (uint32_t)B.nw + (uint32_t)w;
          const uint32_t q = (uint32_t)(ballot >> lx);
          O.bits[g] = (O.neg ? ~q : q) & (O.andv ? O.andv[g] : bitvol_valid(B, w));
        }
      }
      if (O.oz && live) O.oz[idx] = (signed char)(found ? oa : kDistNone);
    } else {
      if (live && x >= O.blo[0] && x <= O.bhi[0] && y >= O.blo[1] && y <= O.bhi[1] && z >= O.blo[2] && z <= O.bhi[2] && !(found && sum == 0)) {
        const size_t at = ((size_t)(z - O.blo[2]) * (size_t)(O.bhi[1] - O.blo[1] + 1) + (size_t)(y - O.blo[1])) * (size_t)(O.bhi[0] - O.blo[0] + 1) +
                          (size_t)(x - O.blo[0]);
        int d2 = found ? sum : INT_MAX, nx = -1, ny = -1, nz = -1;
        if (invert) {                                        // an occupied voxel: to the nearest empty point
          d2 = e2 < d2 ? e2 : d2;
          O.field[at] = -(d2 <= O.max_d2 ? d2 : O.max_d2 + 1);
          nx = x; ny = y; nz = z;
        } else {
          O.field[at] = d2 <= O.max_d2 ? d2 : O.max_d2 + 1;
          if (d2 <= O.max_d2) { nx = x + (int)((best >> 16) & 0xFFu) - 128; ny = y + (int)((best >> 8) & 0xFFu) - 128; nz = z + oa; }
        }
        if (O.nearest) { O.nearest[3 * at] = nx; O.nearest[3 * at + 1] = ny; O.nearest[3 * at + 2] = nz; }
      }
    }
  }
}

// the selected bits of word g: where res differs from occ inside the mask (all = 0), or occ with that difference applied
__device__ __forceinline__ uint32_t dist_selected(const DistBox &B, const uint32_t *occ, const uint32_t *res, uint32_t g, const RegionShape *shapes,
                                                  uint32_t n_shapes, int masked, int all, int *x0, int *y, int *z) {
  const int w = bitvol_word(B, g, x0, y, z);
  uint32_t diff = (occ[g] ^ res[g]) & bitvol_valid(B, w);
  if (masked) diff = bitvol_inside(diff, shapes, n_shapes, *x0, *y, *z);
  return all ? occ[g] ^ diff : diff;
}

__global__ __launch_bounds__(256) void dist_count_kernel(const DistBox B, const uint32_t *occ, const uint32_t *res, const RegionShape *shapes,
                                                        uint32_t n_shapes, int masked, int all, uint32_t *count) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g > B.n_words) return;
  if (g == B.n_words) { count[g] = 0; return; }               // the scan's extra item: its slot receives the total
  int x0, y, z;
  count[g] = (uint32_t)__popc(dist_selected(B, occ, res, g, shapes, n_shapes, masked, all, &x0, &y, &z));
}

// fixed: material + 1 of every new voxel, or 0: that of its nearest voxel of V (xy, oz of the transform of V)
__global__ __launch_bounds__(256) void dist_emit_kernel(const DistBox B, const uint32_t *occ, const uint32_t *res, const RegionShape *shapes,
                                                       uint32_t n_shapes, int masked, int all, const uint32_t *excl, uint32_t fixed,
                                                       const unsigned short *xy, const signed char *oz, const uint32_t *wkeys,
                                                       const uint32_t *wvals, uint32_t n_w, uint32_t *keys, uint32_t *vals) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= B.n_words || excl[g + 1u] == excl[g]) return;
  int x0, y, z;
  uint32_t pos = excl[g];
  const uint32_t o = occ[g];
  const uint32_t plane = (uint32_t)B.ey * (uint32_t)B.nw * 32u;
  for (uint32_t b = dist_selected(B, occ, res, g, shapes, n_shapes, masked, all, &x0, &y, &z); b; b &= b - 1u) {
    const int bit = __ffs((int)b) - 1;
    uint32_t m = fixed;
    if ((o >> bit) & 1u) {
      m = wvals[bitvol_find(wkeys, n_w, region_key(x0 + bit, y, z))];
    } else if (!m) {
      const uint32_t idx = g * 32u + (uint32_t)bit;
      const int dz = oz[idx];                                // within radius2 of V, so there is one
      const unsigned c = xy[(uint32_t)((int)idx + dz * (int)plane)];
      m = wvals[bitvol_find(wkeys, n_w, region_key(x0 + bit + (int)(c & 0xFFu) - 128, y + (int)(c >> 8) - 128, z + dz))];
    }
    keys[pos] = region_key(x0 + bit, y, z); vals[pos] = m;
    pos++;
  }
}

namespace {

const char *kNoMemory = "out of device memory in the distance transform";

// what one round call asks for, validated on the host before anything is queued
struct Request {
  tdt_round r;
  std::vector<RegionShape> shapes;
};

inline int window_of(int r2) { int R = 1; while (R * R < r2) R++; return R; }

int make_request(tdt_ctx *ctx, const tdt_round *r, const tdt_region *regions, size_t n_regions, Request &R) {
  if (!r) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_round pointer");
  if (r->op < TDT_MORPH_DILATE || r->op > TDT_MORPH_SHELL) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_MORPH_* value");
  if (r->radius2 < 1 || r->radius2 > 4096) return fail(ctx, TDT_ERR_INVALID_VALUE, "radius2 must be 1..4096");
  if (r->material < -1 || r->material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be -1 (inherit) or 0..253");
  if (r->border != 0 && r->border != 1) return fail(ctx, TDT_ERR_INVALID_VALUE, "border must be 0 or 1");
  R.r = *r;
  return region_shapes(ctx, regions, n_regions, &R.shapes);
}

// the domain: lo..hi grown by R, clipped to the grid; held to TDT_ROUND_DOMAIN_CAP before anything is allocated over it
int make_domain(tdt_ctx *front, const int lo[3], const int hi[3], int depth, int R, DistBox &B) {
  B.N = 1 << depth; B.R = R;
  int glo[3], ghi[3];
  unsigned long long voxels = 1;
  for (int a = 0; a < 3; a++) {
    glo[a] = lo[a] - R < 0 ? 0 : lo[a] - R;
    ghi[a] = hi[a] + R > B.N - 1 ? B.N - 1 : hi[a] + R;
    voxels *= (unsigned long long)(ghi[a] - glo[a] + 1);
  }
  if (voxels > TDT_ROUND_DOMAIN_CAP)
    return fail(front, TDT_ERR_INVALID_VALUE, "the distance transform's domain holds " + std::to_string(voxels) + " voxels (more than 2^28)");
  bitvol_layout(glo, ghi, B);
  return TDT_OK;
}

// one transform of src (or of its complement): pass x, pass y, pass z into its consumer.  Queued; does not synchronise.
template <int MODE>
void transform(hipStream_t st, const DistBox &B, const uint32_t *src, int invert, signed char *ox, unsigned short *xy, const DistOut &O) {
  const unsigned xt = (unsigned)((B.nw + 1) / 2);
  const unsigned ty = (unsigned)((B.ey + kDistTile - 1) / kDistTile), tz = (unsigned)((B.ez + kDistTile - 1) / kDistTile);
  hipLaunchKernelGGL(dist_pass_x_kernel, dim3(blocks_of((unsigned long long)B.n_words * 32u)), dim3(256), 0, st, B, src, invert, ox);
  hipLaunchKernelGGL(dist_scan_kernel<0>, dim3(xt, ty * (unsigned)B.ez), dim3(256), 0, st, B, invert, (const signed char *)ox,
                     (const unsigned short *)nullptr, xy, O);
  hipLaunchKernelGGL(dist_scan_kernel<MODE>, dim3(xt, tz * (unsigned)B.ey), dim3(256), 0, st, B, invert, (const signed char *)nullptr,
                     (const unsigned short *)xy, (unsigned short *)nullptr, O);
}

// a round op's result on one single-device context, {x, y, z, material + 1} in device memory of ctx (allocated in S; null when
// *n == 0): the whole result, Morton-sorted (delta = false), or only its difference from V, unsorted (delta = true: the FILL
// list of DILATE / CLOSE, the CLEAR list of the others).  Queued on ctx's stream; synchronises.
int round_list(tdt_ctx *front, tdt_ctx *ctx, const Request &R, bool delta, DeviceScratch &S, const int4 **out, uint32_t *n) {
  *out = nullptr; *n = 0;
  const tdt_round &Q = R.r;
  hipStream_t st = ctx->stream;
  int4 *v = nullptr;
  uint32_t nv = 0;
  int depth = 0;
  if (int rc = tree_voxels_capped(front, ctx, S, &v, &nv, &depth)) return rc;
  if (nv == 0) return TDT_OK;                              // every op of the empty set is empty
  int box[6];
  if (int rc = bitvol_list_bbox(front, st, v, nv, depth, S, kNoMemory, "a voxel lies outside the grid", box)) return rc;
  DistBox B;
  if (int rc = make_domain(front, box, box + 3, depth, window_of(Q.radius2), B)) return rc;
  // ---- volumes ----
  const bool grows = Q.op == TDT_MORPH_DILATE || Q.op == TDT_MORPH_CLOSE;
  const bool two = Q.op == TDT_MORPH_OPEN || Q.op == TDT_MORPH_CLOSE;
  const bool inherit = grows && Q.material < 0;
  const size_t padded = (size_t)B.n_words * 32;
  uint32_t *occ = S.get<uint32_t>(B.n_words), *res = S.get<uint32_t>(B.n_words), *mid = two ? S.get<uint32_t>(B.n_words) : nullptr;
  uint32_t *wk = S.get<uint32_t>(nv), *wv = S.get<uint32_t>(nv);
  signed char *ox = S.get<signed char>(padded), *oz = inherit ? S.get<signed char>(padded) : nullptr;
  unsigned short *xy = S.get<unsigned short>(padded), *xy2 = (inherit && two) ? S.get<unsigned short>(padded) : xy;
  if (!occ || !res || (two && !mid) || !wk || !wv || !ox || (inherit && !oz) || !xy || !xy2) return fail(front, TDT_ERR_HIP, kNoMemory);
  RegionShape *d_shapes = nullptr;
  const uint32_t n_shapes = (uint32_t)R.shapes.size();
  if (int rc = upload_shapes(front, st, S, R.shapes.data(), n_shapes, kNoMemory, &d_shapes)) return rc;
  if (int rc = bitvol_rasterise(front, st, v, nv, B, occ, wk, wv)) return rc;
  // ---- the op: W(S) = { d2(q, S) <= radius2 }, C = the complement ----
  DistOut O;
  std::memset(&O, 0, sizeof O);
  O.r2 = Q.radius2;
  switch (Q.op) {
    case TDT_MORPH_DILATE:                                 // W(V)
      O.bits = res; O.oz = oz;
      transform<1>(st, B, occ, 0, ox, xy, O);
      break;
    case TDT_MORPH_ERODE:                                  // V & ~W(C(V))
    case TDT_MORPH_SHELL:                                  // V &  W(C(V))
      O.bits = res; O.andv = occ; O.neg = Q.op == TDT_MORPH_ERODE; O.edge = Q.border == 0;
      transform<1>(st, B, occ, 1, ox, xy, O);
      break;
    case TDT_MORPH_OPEN:                                   // W(V & ~W(C(V))), the outside solid
      O.bits = mid; O.andv = occ; O.neg = 1;
      transform<1>(st, B, occ, 1, ox, xy, O);
      O.bits = res; O.andv = nullptr; O.neg = 0;
      transform<1>(st, B, mid, 0, ox, xy, O);
      break;
    default:                                               // CLOSE: W(V) & ~W(C(W(V))), the outside solid
      O.bits = mid; O.oz = oz;
      transform<1>(st, B, occ, 0, ox, xy, O);
      O.bits = res; O.andv = mid; O.neg = 1; O.oz = nullptr;
      transform<1>(st, B, mid, 1, ox, xy2, O);
      break;
  }
  TDT_HIP(front, hipGetLastError());
  // ---- count, emit, sort ----
  const int all = delta ? 0 : 1, masked = n_shapes ? 1 : 0;
  auto count = [&](uint32_t *cnt) {
    hipLaunchKernelGGL(dist_count_kernel, dim3(blocks_of((size_t)B.n_words + 1)), dim3(256), 0, st, B, (const uint32_t *)occ, (const uint32_t *)res,
                       (const RegionShape *)d_shapes, n_shapes, masked, all, cnt);
  };
  auto emit = [&](const uint32_t *excl, uint32_t *keys, uint32_t *vals) {
    hipLaunchKernelGGL(dist_emit_kernel, dim3(blocks_of(B.n_words)), dim3(256), 0, st, B, (const uint32_t *)occ, (const uint32_t *)res,
                       (const RegionShape *)d_shapes, n_shapes, masked, all, excl, Q.material >= 0 ? (uint32_t)Q.material + 1u : 0u,
                       (const unsigned short *)xy, (const signed char *)oz, (const uint32_t *)wk, (const uint32_t *)wv, nv, keys, vals);
  };
  return bitvol_list_tail(front, st, B.n_words, count, emit, "the result", !delta, nullptr, nullptr, 0u, S, kNoMemory, out, n);
}

struct RoundSource final : VoxelSource {
  const Request &R;
  const bool delta;              // the edit's difference from V, or the extract's whole result
  RoundSource(const Request &r, bool d) : R(r), delta(d) {}
  int run(tdt_ctx *front, tdt_ctx *ctx, int, DeviceScratch &S, const int4 **vox, uint32_t *n) override {
    return round_list(front, ctx, R, delta, S, vox, n);
  }
};

// the signed squared distance over lo..hi on one single-device context, into host memory
int field_one(tdt_ctx *front, tdt_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t max_d2, int32_t border, int32_t *field,
              int32_t *nearest, size_t capacity, size_t *n_voxels) {
  // everything the host can check comes first: the count-only call walks no tree and queues nothing
  int depth = 0;
  if (int rc = walk_inputs(front, ctx, &depth)) return rc;
  DistBox B;
  auto domain = [&] { return make_domain(front, lo, hi, depth, window_of(max_d2), B); };
  if (int rc = bitvol_field_box(front, depth, lo, hi, domain, field != nullptr, capacity, n_voxels)) return rc;
  if (!field) return TDT_OK;
  const size_t count = *n_voxels;
  TDT_HIP(front, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Drain drain{st};
  DeviceScratch S;
  int4 *v = nullptr;
  uint32_t nv = 0;
  if (int rc = tree_voxels_capped(front, ctx, S, &v, &nv, &depth)) { *n_voxels = 0; return rc; }
  const size_t padded = (size_t)B.n_words * 32;
  uint32_t *occ = S.get<uint32_t>(B.n_words), *wk = S.get<uint32_t>(nv), *wv = S.get<uint32_t>(nv);
  signed char *ox = S.get<signed char>(padded);
  unsigned short *xy = S.get<unsigned short>(padded);
  int32_t *d_field = S.get<int32_t>((size_t)count), *d_near = nearest ? S.get<int32_t>(3 * (size_t)count) : nullptr;
  if (!occ || !wk || !wv || !ox || !xy || !d_field || (nearest && !d_near)) return fail(front, TDT_ERR_HIP, kNoMemory);
  if (int rc = bitvol_rasterise(front, st, v, nv, B, occ, wk, wv)) return rc;
  DistOut O;
  std::memset(&O, 0, sizeof O);
  O.field = d_field; O.nearest = d_near; O.max_d2 = max_d2;
  for (int a = 0; a < 3; a++) { O.blo[a] = lo[a]; O.bhi[a] = hi[a]; }
  transform<2>(st, B, occ, 0, ox, xy, O);                  // the empty voxels: to V
  O.edge = border == 0;
  transform<2>(st, B, occ, 1, ox, xy, O);                  // the occupied ones: to the complement
  TDT_HIP(front, hipGetLastError());
  TDT_HIP(front, hipMemcpyAsync(field, d_field, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (nearest) TDT_HIP(front, hipMemcpyAsync(nearest, d_near, 3 * (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  TDT_HIP(front, hipStreamSynchronize(st));
  return TDT_OK;
}

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_morph_round(tdt_ctx *ctx, const tdt_round *r, const tdt_region *regions, size_t n_regions, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  Request R;
  if (int rc = make_request(ctx, r, regions, n_regions, R)) return rc;
  RoundSource src(R, true);
  const bool grows = r->op == TDT_MORPH_DILATE || r->op == TDT_MORPH_CLOSE;
  return region_edit_source(ctx, grows ? TDT_REGION_FILL : TDT_REGION_CLEAR, src, n_cells);
}

int tdt_octree_extract_morph_round(tdt_ctx *ctx, const tdt_round *r, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                                   size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  Request R;
  if (int rc = make_request(ctx, r, regions, n_regions, R)) return rc;
  RoundSource src(R, false);
  return region_extract_source(ctx, src, 0, voxels_xyzm, capacity, n_voxels);
}

int tdt_octree_distance_field(tdt_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t max_d2, int32_t border, int32_t *field,
                              int32_t *nearest_xyz, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  if (!lo || !hi) return fail(ctx, TDT_ERR_INVALID_VALUE, "null box pointer");
  if (max_d2 < 1 || max_d2 > 4096) return fail(ctx, TDT_ERR_INVALID_VALUE, "max_d2 must be 1..4096");
  if (border != 0 && border != 1) return fail(ctx, TDT_ERR_INVALID_VALUE, "border must be 0 or 1");
  return field_one(ctx, first_member(ctx), lo, hi, max_d2, border, field, nearest_xyz, capacity, n_voxels);
}

}  // extern "C"
