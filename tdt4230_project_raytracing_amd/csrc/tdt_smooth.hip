// Voxel smoothing (include/tdt_rt.h tdt_octree_smooth / tdt_octree_extract_smooth / tdt_octree_density_field): the DENSITY
// d(q, S) of every voxel of a domain box — how many voxels of S the ball B(radius2) around q holds — thresholded against the
// ball's SUPPORT n(q) into the next set, step by step; unthresholded it is the density field.
//
// The domain is bbox(V) grown by iterations * R (no growth where a step provably stays inside the box: the header) or the field's
// box grown by R, R = ceil(sqrt(radius2)) <= 15, clipped to the grid and laid out as bitvol_device.hpp describes: x along 32-bit
// words, rows word-aligned in ABSOLUTE x.  One domain serves every iteration.
//
//   bbox, rasterise   tdt_bitvol.hip's: bbox(V); then, per iteration, the occupancy bits of the current list and every voxel's
//              (Morton key, material + 1) for the material lookups.
//   density    smooth_density_kernel<FIELD>.  A block of 4 waves owns a TILE of one word (32 x) by kSmoothTileY by kSmoothTileZ
//              rows and stages in LDS every row the tile and its R-halo in y and z touch, each with one word of halo either
//              side in x: (8 + 2 R)^2 rows of 3 words, 17 KiB at R = 15.  Words beyond the domain read as 0.  A lane is one x of
//              one y of the tile and walks the tile's z.  The count of a voxel is the sum over the ball's (dy, dz) chords of
//              popcount of a window of 2 h + 1 <= 31 bits cut from two adjacent staged words; the chords (their row offset in
//              the staged tile and their half-length h) are a table built on the host and read at a wave-uniform index.  A
//              wave's lanes read at most two words of one row and one of the next, so the LDS serves them as broadcasts.
//              Uniform tiles: when every staged word is 0 the counts are 0, when every one is all-ones (which puts the tile and
//              its halo inside the domain, so inside the grid) they are |B|; the chord loop does not run.
//              A lane keeps the counts of its eight z in registers, so a chord's table word, window and shift are paid once.
//              The support is |B| unless border = 1 (or the field's support array) asks for |(q + B) & G| AND the tile's halo
//              crosses a grid face; there it is the same chord loop over lengths of clipped intervals, in arithmetic.
//                step   FIELD = 0: threshold, mode and mask per voxel; the wave's ballot is two words of the NEXT bit volume;
//                       a block that changed a word raises the step's flag.
//                field  FIELD = 1: the counts (and supports) of the voxels inside the requested box, straight into the result.
//   count, emit  per word popc of the next volume, exclusive_scan_u32, then (Morton key, material + 1) per voxel: a surviving
//              voxel's material by lookup in the sorted keys of the current set, a new one's the fixed one.
//                                                                                   smooth_count_kernel, smooth_emit_kernel
//   inherit    only with material = -1, one lane per padded voxel, the new ones going on: the ball's offsets sorted by
//              (|d|^2, dx, dy, dz) (a host-built table) are walked to the first set bit of the CURRENT volume — the nearest
//              voxel by the header's order — whose material is looked up as above.                   smooth_inherit_kernel
//   tdt_bitvol.hip's tail sorts the pairs and writes the list, which the next iteration rasterises.
//   synchronisations per call: the tree walk, the bounding box; per iteration the step's flag (0: a fixed point, the loop ends),
//   the count, the list.
//   memory     two bit volumes and a count per word of the domain (9 bytes per 32 padded voxels), the tables (<= 60 KiB), and
//              per voxel of the current and the next list what the tail and the sort keep (<= 64 B).
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bitvol_device.hpp"
#include "device_scan.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr int kSmoothTileY = 8;                        // rows of a tile in y: 8 * 32 lanes = one block
constexpr int kSmoothTileZ = 8;                        // rows of a tile in z: a lane's trip count
constexpr int kSmoothMaxR = 15;
constexpr int kSmoothSpan = kSmoothTileY + 2 * kSmoothMaxR;      // staged rows per axis at the largest radius
static_assert(kSmoothTileY * 32 == 256 && kSmoothTileY == kSmoothTileZ, "a block is one tile layer; the halo is the same in y and z");

struct SmoothArgs {            // one launch of the density kernel
  int32_t N, R, ball;          // grid side; window; |B|
  int32_t n_chords;
  int32_t tw0, ty0, tz0;       // the tiles' origin inside the domain: word of a row, row in y, row in z
  int32_t ntw, nty;            // tiles along x and y (blockIdx.x = (tz * nty + ty) * ntw + tw)
  int32_t want_support;        // the support is asked for: border = 1, or the field's support array
  int32_t threshold, mode, masked;   // step
  uint32_t n_shapes;
  int32_t blo[3], bhi[3];      // field: the requested box
};

// a chord of the ball, one word of the host's table: (dz + R) << 26 | (dy + R) << 21 | (its row's offset inside the staged tile) << 8
// | its half-length h
__host__ __device__ __forceinline__ uint32_t smooth_chord(int dy, int dz, int h, int R) {
  const int span = kSmoothTileY + 2 * R;
  return (uint32_t)(dz + R) << 26 | (uint32_t)(dy + R) << 21 | (uint32_t)(((dz + R) * span + (dy + R)) * 3) << 8 | (uint32_t)h;
}

template <int FIELD>
__global__ __launch_bounds__(256) void smooth_density_kernel(const BitBox B, const SmoothArgs A, const uint32_t *src, const uint32_t *chords,
                                                            const RegionShape *shapes, uint32_t *next, uint32_t *changed, int32_t *density,
                                                            int32_t *support) {
  __shared__ uint32_t s[kSmoothSpan * kSmoothSpan * 3];
  const int R = A.R, span = kSmoothTileY + 2 * R;
  const int tw = (int)(blockIdx.x % (uint32_t)A.ntw), tr = (int)(blockIdx.x / (uint32_t)A.ntw);
  const int w = A.tw0 + tw, y0 = A.ty0 + (tr % A.nty) * kSmoothTileY, z0 = A.tz0 + (tr / A.nty) * kSmoothTileZ;
  uint32_t any = 0, holes = 0;
  for (int i = (int)threadIdx.x; i < span * span * 3; i += 256) {
    const int row = i / 3, ww = w - 1 + (i - 3 * row);
    const int yy = y0 - R + row % span, zz = z0 - R + row / span;
    uint32_t v = 0;
    if (yy >= 0 && yy < B.ey && zz >= 0 && zz < B.ez && ww >= 0 && ww < B.nw)
      v = src[((uint32_t)zz * (uint32_t)B.ey + (uint32_t)yy) * (uint32_t)B.nw + (uint32_t)ww];
    s[i] = v;
    any |= v; holes |= ~v;
  }
  const bool some = __syncthreads_or(any != 0u) != 0;        // (also the barrier behind the staging)
  const bool mixed = some && __syncthreads_or(holes != 0u) != 0;
  const int b = (int)(threadIdx.x & 31u), ry = (int)(threadIdx.x >> 5);
  const int x = (B.wx0 + w) * 32 + b, y = B.lo[1] + y0 + ry;
  // does the tile's halo cross a face of the grid?  (block-uniform)
  const bool faces = A.want_support && ((B.wx0 + w) * 32 - R < 0 || (B.wx0 + w) * 32 + 31 + R >= A.N || B.lo[1] + y0 - R < 0 ||
                                        B.lo[1] + y0 + kSmoothTileY - 1 + R >= A.N || B.lo[2] + z0 - R < 0 ||
                                        B.lo[2] + z0 + kSmoothTileZ - 1 + R >= A.N);
  // a lane's column of the tile, all of its z at once: what a chord costs besides its two words and its popcount is paid once
  int dd[kSmoothTileZ], nn[kSmoothTileZ];
#pragma unroll
  for (int rz = 0; rz < kSmoothTileZ; rz++) { dd[rz] = mixed ? 0 : some ? A.ball : 0; nn[rz] = faces ? 0 : A.ball; }
  if (mixed) {
    for (int c = 0; c < A.n_chords; c++) {
      const uint32_t chord = chords[c];
      const int h = (int)(chord & 0xFFu);
      const int first = 32 + b - h;                          // bit of the three-word row where the window starts: 17..63
      const uint32_t window = 0xFFFFFFFFu >> (31 - 2 * h);
      int at = ry * 3 + (int)((chord >> 8) & 0x1FFFu) + (first >> 5);
#pragma unroll
      for (int rz = 0; rz < kSmoothTileZ; rz++) {
        const unsigned long long two = ((unsigned long long)s[at + 1] << 32) | s[at];
        dd[rz] += __popc((uint32_t)(two >> (first & 31)) & window);
        at += span * 3;
      }
    }
  }
  if (faces) {
    for (int c = 0; c < A.n_chords; c++) {
      const uint32_t chord = chords[c];
      const int h = (int)(chord & 0xFFu), yy = y + (int)((chord >> 21) & 31u) - R, zz = B.lo[2] + z0 + (int)(chord >> 26) - R;
      const int x0 = x - h < 0 ? 0 : x - h, x1 = x + h >= A.N ? A.N - 1 : x + h;
      const int len = yy >= 0 && yy < A.N && x0 <= x1 ? x1 - x0 + 1 : 0;
#pragma unroll
      for (int rz = 0; rz < kSmoothTileZ; rz++)
        if (zz + rz >= 0 && zz + rz < A.N) nn[rz] += len;
    }
  }
#pragma unroll
  for (int rz = 0; rz < kSmoothTileZ; rz++) {                // the same trip count in every wave: the ballot below
    const int z = B.lo[2] + z0 + rz;
    const bool live = y0 + ry < B.ey && z0 + rz < B.ez;
    const int base = (rz * span + ry) * 3;
    const int d = dd[rz], n = nn[rz];
    const uint32_t g = ((uint32_t)(z0 + rz) * (uint32_t)B.ey + (uint32_t)(y0 + ry)) * (uint32_t)B.nw + (uint32_t)w;
    if (FIELD) {
      if (live && x >= A.blo[0] && x <= A.bhi[0] && y >= A.blo[1] && y <= A.bhi[1] && z >= A.blo[2] && z <= A.bhi[2]) {
        const size_t at = ((size_t)(z - A.blo[2]) * (size_t)(A.bhi[1] - A.blo[1] + 1) + (size_t)(y - A.blo[1])) * (size_t)(A.bhi[0] - A.blo[0] + 1) +
                          (size_t)(x - A.blo[0]);
        density[at] = d;
        if (support) support[at] = n;
      }
    } else {
      const uint32_t cur_word = s[base + (R * span + R) * 3 + 1];
      const bool cur = (cur_word >> b) & 1u;
      const bool t = A.threshold ? 65536u * (uint32_t)d >= (uint32_t)A.threshold * (uint32_t)n : 2 * d > n;
      bool bit = A.mode == TDT_SMOOTH_BOTH ? t : A.mode == TDT_SMOOTH_ADD ? (cur || t) : (cur && t);
      if (bit != cur && A.masked) {
        bool in = false;
        for (uint32_t k = 0; k < A.n_shapes && !in; k++) in = region_inside(shapes[k], x, y, z);
        if (!in) bit = cur;
      }
      const unsigned long long ballot = __ballot(bit);
      if (live && b == 0) {
        const uint32_t q = (uint32_t)(ballot >> (threadIdx.x & 32u)) & bitvol_valid(B, w);
        next[g] = q;
        if (q != cur_word) *changed = 1u;
      }
    }
  }
}

__global__ __launch_bounds__(256) void smooth_count_kernel(const BitBox B, const uint32_t *res, uint32_t *count) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g > B.n_words) return;
  count[g] = g == B.n_words ? 0u : (uint32_t)__popc(res[g]);  // the scan's extra item: its slot receives the total
}

// fixed: material + 1 of every new voxel, or 0: left to smooth_inherit_kernel
__global__ __launch_bounds__(256) void smooth_emit_kernel(const BitBox B, const uint32_t *occ, const uint32_t *res, const uint32_t *excl,
                                                         uint32_t fixed, const uint32_t *wkeys, const uint32_t *wvals, uint32_t n_w,
                                                         uint32_t *keys, uint32_t *vals) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= B.n_words || excl[g + 1u] == excl[g]) return;
  int x0, y, z;
  bitvol_word(B, g, &x0, &y, &z);
  uint32_t pos = excl[g];
  const uint32_t o = occ[g];
  for (uint32_t bits = res[g]; bits; bits &= bits - 1u) {
    const int bit = __ffs((int)bits) - 1;
    const uint32_t k = region_key(x0 + bit, y, z);
    keys[pos] = k;
    vals[pos] = (o >> bit) & 1u ? wvals[bitvol_find(wkeys, n_w, k)] : fixed;
    pos++;
  }
}

// the new voxels of a step take the material of their nearest voxel of the CURRENT set: offsets = the ball's, sorted by
// (|d|^2, dx, dy, dz), each (dz + 16) << 16 | (dy + 16) << 8 | (dx + 16); one of them hits, because the threshold implies d >= 1
__global__ __launch_bounds__(256) void smooth_inherit_kernel(const BitBox B, const uint32_t *occ, const uint32_t *res, const uint32_t *excl,
                                                            const uint32_t *offsets, uint32_t n_offsets, const uint32_t *wkeys,
                                                            const uint32_t *wvals, uint32_t n_w, uint32_t *vals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;        // one lane per padded voxel: the walks run side by side
  const uint32_t g = i >> 5;
  const int bit = (int)(i & 31u);
  if (g >= B.n_words) return;
  const uint32_t all = res[g];
  if (!((all & ~occ[g]) >> bit & 1u)) return;
  int x0, y, z;
  bitvol_word(B, g, &x0, &y, &z);
  const uint32_t pos = excl[g] + (uint32_t)__popc(all & ((1u << bit) - 1u));
  for (uint32_t k = 0; k < n_offsets; k++) {
    const uint32_t o = offsets[k];
    const int px = x0 + bit + (int)(o & 0xFFu) - 16, py = y + (int)((o >> 8) & 0xFFu) - 16, pz = z + (int)(o >> 16) - 16;
    if (px < B.lo[0] || px > B.hi[0] || py < B.lo[1] || py > B.hi[1] || pz < B.lo[2] || pz > B.hi[2]) continue;
    const uint32_t row = (uint32_t)(pz - B.lo[2]) * (uint32_t)B.ey + (uint32_t)(py - B.lo[1]);
    if ((occ[row * (uint32_t)B.nw + (uint32_t)((px >> 5) - B.wx0)] >> (px & 31)) & 1u) {
      vals[pos] = wvals[bitvol_find(wkeys, n_w, region_key(px, py, pz))];
      return;
    }
  }
}

namespace {

const char *kNoMemory = "out of device memory in the smoothing filter";

inline int window_of(int r2) { int R = 1; while (R * R < r2) R++; return R; }
// the half-length of the ball's chord through (dy, dz), or -1: floor(sqrt(r2 - dy^2 - dz^2))
inline int chord_of(int r2, int dy, int dz) {
  const int rest = r2 - dy * dy - dz * dz;
  if (rest < 0) return -1;
  int h = 0;
  while ((h + 1) * (h + 1) <= rest) h++;
  return h;
}

// the ball of one call as the kernels read it
struct Ball {
  int r2 = 0, R = 0, size = 0;
  std::vector<uint32_t> chords;    // smooth_chord words, dz outer, dy inner
  std::vector<uint32_t> offsets;   // filled on demand: every offset, sorted by (|d|^2, dx, dy, dz)
  explicit Ball(int radius2) : r2(radius2), R(window_of(radius2)) {
    for (int dz = -R; dz <= R; dz++)
      for (int dy = -R; dy <= R; dy++) {
        const int h = chord_of(r2, dy, dz);
        if (h < 0) continue;
        chords.push_back(smooth_chord(dy, dz, h, R));
        size += 2 * h + 1;
      }
  }
  void make_offsets() {
    struct Off { int d2, dx, dy, dz; };
    std::vector<Off> all;
    for (int dx = -R; dx <= R; dx++)
      for (int dy = -R; dy <= R; dy++)
        for (int dz = -R; dz <= R; dz++)
          if (dx * dx + dy * dy + dz * dz <= r2) all.push_back(Off{dx * dx + dy * dy + dz * dz, dx, dy, dz});
    std::sort(all.begin(), all.end(), [](const Off &a, const Off &b) {
      return a.d2 != b.d2 ? a.d2 < b.d2 : a.dx != b.dx ? a.dx < b.dx : a.dy != b.dy ? a.dy < b.dy : a.dz < b.dz;
    });
    for (const Off &o : all) offsets.push_back((uint32_t)(o.dz + 16) << 16 | (uint32_t)(o.dy + 16) << 8 | (uint32_t)(o.dx + 16));
  }
};

// what one smoothing call asks for, validated on the host before anything is queued
struct Request {
  tdt_smooth s;
  std::vector<RegionShape> shapes;
};

int make_request(tdt_ctx *ctx, const tdt_smooth *s, const tdt_region *regions, size_t n_regions, Request &R) {
  if (!s) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_smooth pointer");
  if (s->radius2 < 1 || s->radius2 > 225) return fail(ctx, TDT_ERR_INVALID_VALUE, "radius2 must be 1..225");
  if (s->iterations < 1 || s->iterations > 16) return fail(ctx, TDT_ERR_INVALID_VALUE, "iterations must be 1..16");
  if (s->threshold < 0 || s->threshold > 65536) return fail(ctx, TDT_ERR_INVALID_VALUE, "threshold must be 0 (majority) or 1..65536");
  if (s->mode < TDT_SMOOTH_BOTH || s->mode > TDT_SMOOTH_REMOVE) return fail(ctx, TDT_ERR_INVALID_VALUE, "mode must be a TDT_SMOOTH_* value");
  if (s->material < -1 || s->material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be -1 (inherit) or 0..253");
  if (s->border != 0 && s->border != 1) return fail(ctx, TDT_ERR_INVALID_VALUE, "border must be 0 or 1");
  R.s = *s;
  return region_shapes(ctx, regions, n_regions, &R.shapes);
}

// the domain: lo..hi grown by `grow`, clipped to the grid; held to TDT_SMOOTH_DOMAIN_CAP before anything is allocated over it
int make_domain(tdt_ctx *front, const int lo[3], const int hi[3], int depth, int grow, BitBox &B) {
  const int N = 1 << depth;
  int glo[3], ghi[3];
  unsigned long long voxels = 1;
  for (int a = 0; a < 3; a++) {
    glo[a] = lo[a] - grow < 0 ? 0 : lo[a] - grow;
    ghi[a] = hi[a] + grow > N - 1 ? N - 1 : hi[a] + grow;
    voxels *= (unsigned long long)(ghi[a] - glo[a] + 1);
  }
  if (voxels > TDT_SMOOTH_DOMAIN_CAP)
    return fail(front, TDT_ERR_INVALID_VALUE, "the smoothing filter's domain holds " + std::to_string(voxels) + " voxels (more than 2^28)");
  bitvol_layout(glo, ghi, B);
  return TDT_OK;
}

// the tables of a ball in device memory
int upload_words(tdt_ctx *front, hipStream_t st, DeviceScratch &S, const std::vector<uint32_t> &h, uint32_t **d) {
  *d = S.get<uint32_t>(h.size());
  if (!*d) return fail(front, TDT_ERR_HIP, kNoMemory);
  TDT_HIP(front, hipMemcpyAsync(*d, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  return TDT_OK;
}

// the tiles that cover words w0..w1 of a row and rows y0..y1, z0..z1 of the domain, and the launch over them
template <int FIELD>
void launch_density(hipStream_t st, const BitBox &B, SmoothArgs A, int w0, int w1, int y0, int y1, int z0, int z1, const uint32_t *src,
                    const uint32_t *chords, const RegionShape *shapes, uint32_t *next, uint32_t *changed, int32_t *density, int32_t *support) {
  A.tw0 = w0; A.ty0 = y0; A.tz0 = z0;
  A.ntw = w1 - w0 + 1; A.nty = (y1 - y0) / kSmoothTileY + 1;
  const unsigned ntz = (unsigned)((z1 - z0) / kSmoothTileZ + 1);
  hipLaunchKernelGGL(smooth_density_kernel<FIELD>, dim3((unsigned)A.ntw * (unsigned)A.nty * ntz), dim3(256), 0, st, B, A, src, chords, shapes, next,
                     changed, density, support);
}

// the smoothed set on one single-device context, {x, y, z, material + 1} Morton-sorted in device memory of ctx (null when
// *n == 0).  The list lives in S or in *held, which the caller keeps until it is done with it.  Queued on ctx's stream; synchronises.
int smooth_list(tdt_ctx *front, tdt_ctx *ctx, const Request &Q, DeviceScratch &S, std::unique_ptr<DeviceScratch> &held, const int4 **out,
                uint32_t *n, int *depth_out) {
  *out = nullptr; *n = 0;
  const tdt_smooth &P = Q.s;
  hipStream_t st = ctx->stream;
  int4 *v = nullptr;
  uint32_t nv = 0;
  int depth = 0;
  if (int rc = tree_voxels_capped(front, ctx, S, &v, &nv, &depth)) return rc;
  *depth_out = depth;
  if (nv == 0) return TDT_OK;                              // no voxel, no density: the empty set stays empty
  int box[6];
  if (int rc = bitvol_list_bbox(front, st, v, nv, depth, S, kNoMemory, "a voxel lies outside the grid", box)) return rc;
  Ball ball(P.radius2);
  // with the outside counted as empty, a majority (and any fraction above one half) never leaves the bounding box
  const bool stays = P.border == 0 && (P.threshold == 0 || P.threshold > 32768);
  BitBox B;
  if (int rc = make_domain(front, box, box + 3, depth, stays ? 0 : P.iterations * ball.R, B)) return rc;
  // ---- volumes and tables ----
  const bool inherit = P.material < 0 && P.mode != TDT_SMOOTH_REMOVE;
  uint32_t *occ = S.get<uint32_t>(B.n_words), *res = S.get<uint32_t>(B.n_words), *flag = S.get<uint32_t>(1);
  uint32_t *d_chords = nullptr, *d_offsets = nullptr;
  if (!occ || !res || !flag) return fail(front, TDT_ERR_HIP, kNoMemory);
  if (int rc = upload_words(front, st, S, ball.chords, &d_chords)) return rc;
  if (inherit) {
    ball.make_offsets();
    if (int rc = upload_words(front, st, S, ball.offsets, &d_offsets)) return rc;
  }
  RegionShape *d_shapes = nullptr;
  const uint32_t n_shapes = (uint32_t)Q.shapes.size();
  if (int rc = upload_shapes(front, st, S, Q.shapes.data(), n_shapes, kNoMemory, &d_shapes)) return rc;
  SmoothArgs A;
  std::memset(&A, 0, sizeof A);
  A.N = 1 << depth; A.R = ball.R; A.ball = ball.size; A.n_chords = (int32_t)ball.chords.size();
  A.want_support = P.border; A.threshold = P.threshold; A.mode = P.mode; A.masked = n_shapes ? 1 : 0; A.n_shapes = n_shapes;
  // ---- the steps ----
  const int4 *cur = v;
  uint32_t n_cur = nv;
  for (int it = 0; it < P.iterations && n_cur; it++) {
    std::unique_ptr<DeviceScratch> T(new DeviceScratch);   // this step's keys and its list
    uint32_t *wk = T->get<uint32_t>(n_cur), *wv = T->get<uint32_t>(n_cur);
    if (!wk || !wv) return fail(front, TDT_ERR_HIP, kNoMemory);
    if (int rc = bitvol_rasterise(front, st, cur, n_cur, B, occ, wk, wv)) return rc;
    TDT_HIP(front, hipMemsetAsync(flag, 0, sizeof(uint32_t), st));
    launch_density<0>(st, B, A, 0, B.nw - 1, 0, B.ey - 1, 0, B.ez - 1, occ, d_chords, d_shapes, res, flag, nullptr, nullptr);
    TDT_HIP(front, hipGetLastError());
    uint32_t changed = 0;
    if (int rc = read_word(front, st, flag, &changed)) return rc;
    if (!changed) break;                                   // a fixed point: every later step leaves it too
    auto count = [&](uint32_t *cnt) {
      hipLaunchKernelGGL(smooth_count_kernel, dim3(blocks_of((size_t)B.n_words + 1)), dim3(256), 0, st, B, (const uint32_t *)res, cnt);
    };
    auto emit = [&](const uint32_t *excl, uint32_t *keys, uint32_t *vals) {
      hipLaunchKernelGGL(smooth_emit_kernel, dim3(blocks_of(B.n_words)), dim3(256), 0, st, B, (const uint32_t *)occ, (const uint32_t *)res, excl,
                         P.material >= 0 ? (uint32_t)P.material + 1u : 0u, (const uint32_t *)wk, (const uint32_t *)wv, n_cur, keys, vals);
      if (inherit)
        hipLaunchKernelGGL(smooth_inherit_kernel, dim3(blocks_of((unsigned long long)B.n_words * 32u)), dim3(256), 0, st, B, (const uint32_t *)occ, (const uint32_t *)res, excl,
                           (const uint32_t *)d_offsets, (uint32_t)ball.offsets.size(), (const uint32_t *)wk, (const uint32_t *)wv, n_cur, vals);
    };
    const int4 *nxt = nullptr;
    uint32_t n_nxt = 0;
    if (int rc = bitvol_list_tail(front, st, B.n_words, count, emit, "the result", true, nullptr, nullptr, 0u, *T, kNoMemory, &nxt, &n_nxt)) return rc;
    held = std::move(T);                                   // the tail has synchronised: the step before this one's goes
    cur = nxt; n_cur = n_nxt;
  }
  *out = n_cur ? cur : nullptr; *n = n_cur;
  return TDT_OK;
}

// one single-device context: the edit (n_cells) or, host_out / n_out, the result into host memory
int smooth_one(tdt_ctx *front, tdt_ctx *ctx, const Request &Q, uint32_t *n_cells, bool extract, int32_t *host_out, size_t capacity, size_t *n_out) {
  TDT_HIP(front, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DeviceScratch S;
  std::unique_ptr<DeviceScratch> held;
  Drain drain{st};                                         // before anything above is freed
  const int4 *res = nullptr;
  uint32_t n_res = 0;
  int depth = 0;
  if (int rc = smooth_list(front, ctx, Q, S, held, &res, &n_res, &depth)) return rc;
  if (extract) return list_to_host(front, st, res, n_res, sizeof(int4), "voxels", host_out, capacity, n_out);
  return rebuild_install(front, ctx, res, n_res, depth, true, n_cells, [&] { held.reset(); S.release(); });
}

// the density over lo..hi on one single-device context, into host memory
int field_one(tdt_ctx *front, tdt_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t radius2, int32_t *density, int32_t *support,
              size_t capacity, size_t *n_voxels) {
  // everything the host can check comes first: the count-only call walks no tree and queues nothing
  int depth = 0;
  if (int rc = walk_inputs(front, ctx, &depth)) return rc;
  Ball ball(radius2);
  BitBox B;
  auto domain = [&] { return make_domain(front, lo, hi, depth, ball.R, B); };
  if (int rc = bitvol_field_box(front, depth, lo, hi, domain, density != nullptr, capacity, n_voxels)) return rc;
  if (!density) return TDT_OK;
  const size_t count = *n_voxels;
  TDT_HIP(front, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Drain drain{st};
  DeviceScratch S;
  int4 *v = nullptr;
  uint32_t nv = 0;
  if (int rc = tree_voxels_capped(front, ctx, S, &v, &nv, &depth)) { *n_voxels = 0; return rc; }
  uint32_t *occ = S.get<uint32_t>(B.n_words), *wk = S.get<uint32_t>(nv), *wv = S.get<uint32_t>(nv), *d_chords = nullptr;
  int32_t *d_density = S.get<int32_t>(count), *d_support = support ? S.get<int32_t>(count) : nullptr;
  if (!occ || !wk || !wv || !d_density || (support && !d_support)) return fail(front, TDT_ERR_HIP, kNoMemory);
  if (int rc = upload_words(front, st, S, ball.chords, &d_chords)) return rc;
  if (int rc = bitvol_rasterise(front, st, v, nv, B, occ, wk, wv)) return rc;
  SmoothArgs A;
  std::memset(&A, 0, sizeof A);
  A.N = 1 << depth; A.R = ball.R; A.ball = ball.size; A.n_chords = (int32_t)ball.chords.size();
  A.want_support = support ? 1 : 0;
  for (int a = 0; a < 3; a++) { A.blo[a] = lo[a]; A.bhi[a] = hi[a]; }
  launch_density<1>(st, B, A, (lo[0] >> 5) - B.wx0, (hi[0] >> 5) - B.wx0, lo[1] - B.lo[1], hi[1] - B.lo[1], lo[2] - B.lo[2], hi[2] - B.lo[2], occ,
                    d_chords, nullptr, nullptr, nullptr, d_density, d_support);
  TDT_HIP(front, hipGetLastError());
  TDT_HIP(front, hipMemcpyAsync(density, d_density, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (support) TDT_HIP(front, hipMemcpyAsync(support, d_support, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  TDT_HIP(front, hipStreamSynchronize(st));
  return TDT_OK;
}

}  // namespace
}  // namespace tdt

extern "C" {

int32_t tdt_ball_size(int32_t radius2) {
  if (radius2 < 1 || radius2 > 4096) return -1;
  const int R = tdt::window_of(radius2);
  int32_t size = 0;
  for (int dz = -R; dz <= R; dz++)
    for (int dy = -R; dy <= R; dy++) {
      const int h = tdt::chord_of(radius2, dy, dz);
      if (h >= 0) size += 2 * h + 1;
    }
  return size;
}

int tdt_octree_smooth(tdt_ctx *ctx, const tdt_smooth *s, const tdt_region *regions, size_t n_regions, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  Request Q;
  if (int rc = make_request(ctx, s, regions, n_regions, Q)) return rc;
  // every replica, as region edits do, a misfit reporting the size to grow to
  return edit_replicas(ctx, true, n_cells, [&](tdt_ctx *mem, uint32_t *nc) { return smooth_one(ctx, mem, Q, nc, false, nullptr, 0, nullptr); });
}

int tdt_octree_extract_smooth(tdt_ctx *ctx, const tdt_smooth *s, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                              size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  Request Q;
  if (int rc = make_request(ctx, s, regions, n_regions, Q)) return rc;
  return smooth_one(ctx, first_member(ctx), Q, nullptr, true, voxels_xyzm, capacity, n_voxels);
}

int tdt_octree_density_field(tdt_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t radius2, int32_t *density, int32_t *support,
                             size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  if (!lo || !hi) return fail(ctx, TDT_ERR_INVALID_VALUE, "null box pointer");
  if (radius2 < 1 || radius2 > 225) return fail(ctx, TDT_ERR_INVALID_VALUE, "radius2 must be 1..225");
  return field_one(ctx, first_member(ctx), lo, hi, radius2, density, support, capacity, n_voxels);
}

}  // extern "C"
