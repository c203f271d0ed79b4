// Voxel extraction and in-place compaction — the steps octree_update.comp leaves as TODOs (uc:86-94: "implement removing
// cell if it is empty after removing", "implement removing hierarchies when emptying nodes"), as explicit operations:
// tdt_octree_census / tdt_octree_extract / tdt_octree_compact (include/tdt_rt.h).
//
// The walk is the LOGICAL tree treeLookup resolves (rc:372-393): node index = 8 * cell + child digit (x*4 + y*2 + z) from
// cell 0 for max_depth levels; EMPTY (0) -> nothing; LEAF (2) -> the whole block under the node, material = value; any other
// type -> descend into cell `value`, except on level max_depth, where the loop ends; nodes past the buffer read as zero.
// Bounded by max_depth, so a cycle cannot loop, and a shared cell is walked once per path that reaches it.
//
//   per level l = 1 .. D, over a frontier of (cell, Morton key of its block) items:
//     classify  8 lanes per item read the cell's 8 nodes (one 64-byte line) and ballot them into a child and a leaf mask
//     scan      two exclusive prefix sums over the per-item child / leaf counts -> output offsets
//     emit      the same lanes write the next frontier (in key order) and the leaf records (start key at level D, value, l)
//   ONE host synchronisation reads the totals (census); extraction then sorts the leaf records by start key (the builder's
//   radix sort), prefix-sums their 8^(D-l) voxel counts and expands them, one lane per voxel, into {x, y, z, value + 1}:
//   each block is a contiguous range of Morton keys, so the list comes out sorted.  Compaction feeds that list to the
//   builder (build_cells_device) and copies the canonical tree over the bound buffer.
//
// Kernel launches are sized on the host by a frontier capacity per level (min(8^(l-1), cells in the buffer + 1): a tree
// reaches every in-buffer cell at most once), and every kernel reads the real count from device memory.  Shared cells can
// overflow that: the walk then records the true counts of the levels it got through and runs again with room for them.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "device_scan.hpp"
#include "region_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr int kMaxWalkDepth = 10;            // the builder's range: Morton keys of 3 * 10 bits

struct WalkMeta {                            // device-side bookkeeping of one walk (zeroed, then count[1] = 1: the root)
  uint32_t count[kMaxWalkDepth + 2];         // frontier items of level l (clamped to the capacity)
  uint32_t true_count[kMaxWalkDepth + 2];    // ... before clamping
  unsigned long long leaf_base[kMaxWalkDepth + 2];   // leaf records of the levels before l
  unsigned long long reach, leaves, voxels;
  uint32_t max_leaf, max_cell;               // largest LEAF value met, largest cell index descended into
  uint32_t overflow_level, leaf_overflow;    // first level whose frontier did not fit; leaf records did not fit
};

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64); v = t > v ? t : v; }
  return v;
}

__device__ __forceinline__ uint2 load_node(const uint2 *nodes, unsigned long long n_nodes, uint32_t cell, uint32_t c) {
  const unsigned long long k = (unsigned long long)cell * 8ull + c;
  return k < n_nodes ? nodes[k] : make_uint2(0u, 0u);           // the robust access: past the end reads as zero (EMPTY)
}

// lanes 8 * i + c for items i <= cap (item cap and items past the count write zeros: the scans run over cap + 1 entries)
__global__ __launch_bounds__(256) void compact_classify_kernel(const uint2 *nodes, unsigned long long n_nodes, const uint32_t *f_cell,
                                                              const uint32_t *f_count, uint32_t cap, int last, uint32_t *mask, uint32_t *cc,
                                                              uint32_t *lc, WalkMeta *M) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, i = t >> 3, c = t & 7u;
  const uint32_t n = *f_count;
  const bool live = i < n;
  const uint32_t cell = live ? f_cell[i] : 0u;
  const uint2 nd = live ? load_node(nodes, n_nodes, cell, c) : make_uint2(0u, 0u);
  const bool leaf = live && nd.y == 2u;
  const bool child = live && !last && nd.y != 0u && nd.y != 2u;
  const unsigned long long bl = __ballot(leaf), bc = __ballot(child);
  const uint32_t sh = threadIdx.x & 56u;                     // the item's 8 lanes within the wave
  if (c == 0 && i <= cap) {
    const uint32_t lm = (uint32_t)(bl >> sh) & 0xFFu, cm = (uint32_t)(bc >> sh) & 0xFFu;
    mask[i] = cm | (lm << 8);
    cc[i] = (uint32_t)__popc(cm);
    lc[i] = (uint32_t)__popc(lm);
  }
  const uint32_t mv = wave_max_u32(leaf ? nd.x : 0u), mc = wave_max_u32(live && c == 0 ? cell : 0u);
  if ((threadIdx.x & 63u) == 0) {
    if (mv) atomicMax(&M->max_leaf, mv);
    if (mc) atomicMax(&M->max_cell, mc);
  }
}

// leaf_start == null: a census, no leaf records
__global__ __launch_bounds__(256) void compact_emit_kernel(const uint2 *nodes, unsigned long long n_nodes, const uint32_t *f_cell,
                                                          const uint32_t *f_key, uint32_t cap, const uint32_t *mask, const uint32_t *coff,
                                                          const uint32_t *loff, uint32_t *n_cell, uint32_t *n_key, uint32_t n_cap,
                                                          uint32_t *leaf_start, uint32_t *leaf_val, uint8_t *leaf_lvl,
                                                          unsigned long long leaf_cap, int level, int depth, WalkMeta *M) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, i = t >> 3, c = t & 7u;
  const uint32_t n = M->count[level];
  const unsigned long long base = M->leaf_base[level];
  if (t == 0) {                                             // the level's totals (nothing else reads these words in this launch)
    const uint32_t nc = coff[cap], nl = loff[cap];
    M->true_count[level + 1] = nc;
    M->count[level + 1] = nc < n_cap ? nc : n_cap;
    if (nc > n_cap && M->overflow_level == 0u) M->overflow_level = (uint32_t)level + 1u;
    M->leaf_base[level + 1] = base + nl;
    if (leaf_start && base + nl > leaf_cap) M->leaf_overflow = 1u;
    M->reach += n; M->leaves += nl; M->voxels += (unsigned long long)nl << (3 * (depth - level));
  }
  if (i >= n) return;
  const uint32_t m = mask[i], below = (1u << c) - 1u;
  const uint32_t cm = m & 0xFFu, lm = (m >> 8) & 0xFFu;
  if (!(((cm | lm) >> c) & 1u)) return;
  const uint2 nd = load_node(nodes, n_nodes, f_cell[i], c);
  const uint32_t key = (f_key[i] << 3) | c;
  if ((cm >> c) & 1u) {
    const uint32_t pos = coff[i] + (uint32_t)__popc(cm & below);
    if (pos < n_cap) { n_cell[pos] = nd.x; n_key[pos] = key; }
  } else if (leaf_start) {
    const unsigned long long pos = base + loff[i] + (uint32_t)__popc(lm & below);
    if (pos < leaf_cap) { leaf_start[pos] = key << (3 * (depth - level)); leaf_val[pos] = nd.x; leaf_lvl[pos] = (uint8_t)level; }
  }
}

__global__ __launch_bounds__(256) void compact_iota_kernel(uint32_t *v, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) v[i] = i;
}

// voxels of each sorted leaf record (entry n = 0, so an exclusive scan over n + 1 leaves the total in [n])
__global__ __launch_bounds__(256) void compact_counts_kernel(const uint32_t *order, const uint8_t *leaf_lvl, uint32_t n, int depth, uint32_t *vc) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  vc[i] = i < n ? 1u << (3 * (depth - (int)leaf_lvl[order[i]])) : 0u;
}

// one lane per voxel: its leaf record is the last one whose voxel offset is <= the lane (offsets strictly increase)
__global__ __launch_bounds__(256) void compact_expand_kernel(const uint32_t *start, const uint32_t *order, const uint32_t *voff, uint32_t n_leaves,
                                                            const uint32_t *leaf_val, uint32_t n_vox, int4 *out) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= n_vox) return;
  uint32_t lo = 0, hi = n_leaves;                           // invariant: voff[lo] <= v < voff[hi]
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (voff[mid] <= v) lo = mid; else hi = mid; }
  const uint32_t key = start[lo] + (v - voff[lo]);
  out[v] = region_voxel(key, (int)(leaf_val[order[lo]] + 1u));
}

// the bound slots 0 / 7 of ctx (a single-device context); errors are reported on `front`
int walk_inputs(tdt_ctx *front, tdt_ctx *ctx, int *depth) {
  if (!ctx->ssbo[TDT_SLOT_CELLS]) return fail(front, TDT_ERR_INCOMPLETE, "no buffer bound to shader-storage slot 0");
  if (!ctx->ssbo[TDT_SLOT_OCTREE_INTS]) return fail(front, TDT_ERR_INCOMPLETE, "no buffer bound to shader-storage slot 7");
  if (ctx->ssbo[TDT_SLOT_OCTREE_INTS]->bytes < 4) return fail(front, TDT_ERR_INVALID_VALUE, "octree uniform buffer (slot 7) is too small");
  int32_t d = 0;
  std::memcpy(&d, ctx->ssbo[TDT_SLOT_OCTREE_INTS]->shadow, sizeof d);
  if (d < 1 || d > kMaxWalkDepth) return fail(front, TDT_ERR_INVALID_VALUE, "max_depth must be 1..10 to walk the tree");
  *depth = d;
  return TDT_OK;
}

namespace {

using Scratch = DeviceScratch;
const char *kNoMemory = "out of device memory in the octree walk";

struct Walk {
  WalkMeta meta;
  int depth = 0;
  uint64_t buffer_cells = 0;
  int64_t counter = -1;
  // leaf records (extraction only), valid until the Walk dies
  Scratch mem;
  uint32_t *leaf_start = nullptr, *leaf_val = nullptr; uint8_t *leaf_lvl = nullptr;
  uint32_t n_leaves = 0;
};

// the level-by-level walk of the bound tree; leaves = keep the leaf records for an expansion.  One host synchronisation,
// unless shared cells overflow the frontier capacities (then once more per retry).
int walk_tree(tdt_ctx *front, tdt_ctx *ctx, bool leaves, Walk &W) {
  int D = 0;
  if (int rc = walk_inputs(front, ctx, &D)) return rc;
  const tdt_buffer *cb = ctx->ssbo[TDT_SLOT_CELLS];
  const uint2 *nodes = (const uint2 *)cb->dev;
  const unsigned long long n_nodes = cb->bytes / 8;
  W.depth = D; W.buffer_cells = cb->bytes / 64;
  const tdt_buffer *counter = ctx->atomic0 && ctx->atomic0->bytes >= 4 ? ctx->atomic0 : nullptr;
  hipStream_t st = ctx->stream;
  TDT_HIP(front, hipSetDevice(ctx->device));
  // frontier capacity per level (items of level l live in cells read at level l)
  const unsigned long long tree_room = W.buffer_cells + 1;
  std::vector<unsigned long long> cap(D + 2, 0);
  for (int l = 1; l <= D; l++) { const unsigned long long full = 1ull << (3 * (l - 1)); cap[l] = full < tree_room ? full : tree_room; }
  unsigned long long leaf_cap = 8ull * tree_room;
  for (int attempt = 0;; attempt++) {
    W.mem.release();
    unsigned long long fmax = 0, fsum = 0;
    for (int l = 1; l <= D; l++) { fmax = cap[l] > fmax ? cap[l] : fmax; fsum += cap[l]; }
    if (fmax >= (1ull << 28)) return fail(front, TDT_ERR_INVALID_VALUE, "tree too large to walk");
    if (leaf_cap > 8ull * fsum) leaf_cap = 8ull * fsum;
    Scratch &S = W.mem;
    uint32_t *f_cell[2] = {S.get<uint32_t>(fmax), S.get<uint32_t>(fmax)}, *f_key[2] = {S.get<uint32_t>(fmax), S.get<uint32_t>(fmax)};
    uint32_t *mask = S.get<uint32_t>(fmax + 1), *cc = S.get<uint32_t>(fmax + 1), *lc = S.get<uint32_t>(fmax + 1);
    uint32_t *scr = S.get<uint32_t>(scan_scratch_words(fmax + 1));
    WalkMeta *dm = S.get<WalkMeta>(1);
    uint32_t *ls = nullptr, *lv = nullptr; uint8_t *ll = nullptr;
    if (leaves) { ls = S.get<uint32_t>(leaf_cap); lv = S.get<uint32_t>(leaf_cap); ll = S.get<uint8_t>(leaf_cap); }
    if (!f_cell[0] || !f_cell[1] || !f_key[0] || !f_key[1] || !mask || !cc || !lc || !scr || !dm || (leaves && (!ls || !lv || !ll)))
      return fail(front, TDT_ERR_HIP, kNoMemory);
    WalkMeta init;
    std::memset(&init, 0, sizeof init);
    init.count[1] = init.true_count[1] = 1;
    TDT_HIP(front, hipMemcpyAsync(dm, &init, sizeof init, hipMemcpyHostToDevice, st));
    TDT_HIP(front, hipMemsetAsync(f_cell[0], 0, sizeof(uint32_t), st));      // the root: cell 0, key 0
    TDT_HIP(front, hipMemsetAsync(f_key[0], 0, sizeof(uint32_t), st));
    for (int l = 1; l <= D; l++) {
      const int a = (l - 1) & 1, b = a ^ 1;
      const uint32_t c = (uint32_t)cap[l], nc = (uint32_t)(l < D ? cap[l + 1] : 0);
      const unsigned g = blocks_of(8ull * ((unsigned long long)c + 1));
      hipLaunchKernelGGL(compact_classify_kernel, dim3(g), dim3(256), 0, st, nodes, n_nodes, (const uint32_t *)f_cell[a],
                         (const uint32_t *)(&dm->count[l]), c, l == D ? 1 : 0, mask, cc, lc, dm);
      TDT_HIP(front, exclusive_scan_u32(st, cc, cc, c + 1u, scr));
      TDT_HIP(front, exclusive_scan_u32(st, lc, lc, c + 1u, scr));
      hipLaunchKernelGGL(compact_emit_kernel, dim3(g), dim3(256), 0, st, nodes, n_nodes, (const uint32_t *)f_cell[a], (const uint32_t *)f_key[a], c,
                         (const uint32_t *)mask, (const uint32_t *)cc, (const uint32_t *)lc, f_cell[b], f_key[b], nc, ls, lv, ll, leaf_cap, l, D, dm);
    }
    TDT_HIP(front, hipGetLastError());
    uint32_t cword = 0;
    TDT_HIP(front, hipMemcpyAsync(&W.meta, dm, sizeof W.meta, hipMemcpyDeviceToHost, st));
    if (counter) TDT_HIP(front, hipMemcpyAsync(&cword, counter->dev, sizeof cword, hipMemcpyDeviceToHost, st));
    TDT_HIP(front, hipStreamSynchronize(st));             // the one thing the host must know: the totals
    W.counter = counter ? (int64_t)cword : -1;
    const WalkMeta &M = W.meta;
    if (!M.overflow_level && !M.leaf_overflow) {
      W.leaf_start = ls; W.leaf_val = lv; W.leaf_lvl = ll; W.n_leaves = (uint32_t)M.leaves;
      return TDT_OK;
    }
    if (attempt >= D + 1) return fail(front, TDT_ERR_HIP, "octree walk: frontier capacities did not converge");
    if (M.overflow_level) {                               // levels up to the first overflow are exact; room for 8x beyond
      const int lo = (int)M.overflow_level;
      for (int l = 2; l <= lo; l++) cap[l] = cap[l] > M.true_count[l] ? cap[l] : M.true_count[l];
      for (int l = lo + 1; l <= D; l++) {
        const unsigned long long full = 1ull << (3 * (l - 1)), grow = 8ull * cap[l - 1];
        const unsigned long long want = grow < full ? grow : full;
        cap[l] = cap[l] > want ? cap[l] : want;
      }
      leaf_cap = ~0ull;                                   // (clamped to 8 per frontier item above)
    } else {
      leaf_cap = M.leaves;                                // frontiers were exact: so is the leaf total
    }
  }
}

// the sorted voxel list of a finished walk (leaves kept) into device memory: n = W.meta.voxels entries of 4 x int32
int expand_voxels(tdt_ctx *front, tdt_ctx *ctx, Walk &W, Scratch &S, int4 **out) {
  hipStream_t st = ctx->stream;
  const uint32_t n = W.n_leaves, nv = (uint32_t)W.meta.voxels;
  uint32_t *order = S.get<uint32_t>(n), *k_alt = S.get<uint32_t>(n), *v_alt = S.get<uint32_t>(n);
  uint32_t *hist = S.get<uint32_t>(sort_hist_words(n)), *hscr = S.get<uint32_t>(sort_scratch_words(n));
  uint32_t *voff = S.get<uint32_t>((size_t)n + 1), *vscr = S.get<uint32_t>(scan_scratch_words((size_t)n + 1));
  int4 *vox = S.get<int4>(nv);
  if (!order || !k_alt || !v_alt || !hist || !hscr || !voff || !vscr || !vox) return fail(front, TDT_ERR_HIP, kNoMemory);
  uint32_t *key = W.leaf_start;                            // sorted in place (the walk's array, or its scratch twin)
  hipLaunchKernelGGL(compact_iota_kernel, dim3(blocks_of(n)), dim3(256), 0, st, order, n);
  TDT_HIP(front, sort_pairs_u32(st, key, order, k_alt, v_alt, n, hist, hscr));
  hipLaunchKernelGGL(compact_counts_kernel, dim3(blocks_of((unsigned long long)n + 1)), dim3(256), 0, st, (const uint32_t *)order,
                     (const uint8_t *)W.leaf_lvl, n, W.depth, voff);
  TDT_HIP(front, exclusive_scan_u32(st, voff, voff, n + 1u, vscr));
  hipLaunchKernelGGL(compact_expand_kernel, dim3(blocks_of(nv)), dim3(256), 0, st, (const uint32_t *)key, (const uint32_t *)order,
                     (const uint32_t *)voff, n, (const uint32_t *)W.leaf_val, nv, vox);
  TDT_HIP(front, hipGetLastError());
  *out = vox;
  return TDT_OK;
}

}  // namespace

int tree_voxels(tdt_ctx *front, tdt_ctx *ctx, uint32_t leaf_limit, DeviceScratch &S, int4 **out, uint32_t *n, int *depth) {
  *out = nullptr; *n = 0;
  Walk W;
  if (int rc = walk_tree(front, ctx, true, W)) return rc;
  *depth = W.depth;
  if (W.meta.leaves && W.meta.max_leaf >= leaf_limit)
    return fail(front, TDT_ERR_INVALID_VALUE, leaf_limit == 254u ? "a LEAF value >= 254 cannot be rebuilt (the builder's materials are 0..253)"
                                                                 : "a LEAF value >= 2^31 - 1 does not fit the voxel list");
  if (W.meta.voxels == 0) return TDT_OK;
  if (int rc = expand_voxels(front, ctx, W, S, out)) return rc;
  *n = (uint32_t)W.meta.voxels;
  return TDT_OK;                                          // the walk's leaf records are freed here: they are in *out now
}

int install_cells(tdt_ctx *front, tdt_ctx *ctx, tdt_buffer *built, uint32_t nc) {
  tdt_buffer *cb = ctx->ssbo[TDT_SLOT_CELLS];
  hipStream_t st = ctx->stream;
  const size_t bytes = (size_t)nc * 64;
  if (bytes > cb->bytes) {
    if (built) tdt_buffer_destroy(built);
    return fail(front, TDT_ERR_INVALID_VALUE, "the canonical tree (" + std::to_string(nc) + " cells) does not fit in the cells buffer (" +
                                                  std::to_string(cb->bytes / 64) + " cells)");
  }
  hipError_t e = built ? hipMemcpyAsync(cb->dev, built->dev, bytes, hipMemcpyDeviceToDevice, st) : hipMemsetAsync(cb->dev, 0, bytes, st);
  if (e == hipSuccess && cb->bytes > bytes) e = hipMemsetAsync((char *)cb->dev + bytes, 0, cb->bytes - bytes, st);
  tdt_buffer *counter = ctx->atomic0 && ctx->atomic0->bytes >= 4 ? ctx->atomic0 : nullptr;
  if (e == hipSuccess && counter) e = hipMemsetD32Async((hipDeviceptr_t)counter->dev, (int)nc, 1, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);       // (the rebuilt tree is freed below)
  if (e != hipSuccess) { if (built) tdt_buffer_destroy(built); return hip_fail(front, e, "octree compaction"); }
  // every derived table of the cells buffer (LDS image, whole-depth table, bricks, pixel costs) is keyed on its version
  std::memset(cb->shadow, 0, sizeof cb->shadow);
  if (built) std::memcpy(cb->shadow, built->shadow, sizeof cb->shadow < bytes ? sizeof cb->shadow : bytes);
  cb->version += 0x100000000ull;
  if (counter) { std::memcpy(counter->shadow, &nc, sizeof nc); counter->version += 0x100000000ull; }
  if (built) tdt_buffer_destroy(built);
  return TDT_OK;
}

namespace {

// compaction of one single-device context
int compact_one(tdt_ctx *front, tdt_ctx *ctx, uint32_t *n_cells) {
  Scratch S;
  int4 *vox = nullptr;
  uint32_t nv = 0;
  int depth = 0;
  if (int rc = tree_voxels(front, ctx, 254u, S, &vox, &nv, &depth)) return rc;
  return rebuild_install(front, ctx, vox, nv, depth, false, n_cells, [&] { S.release(); });   // *n_cells only once installed
}

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_census(tdt_ctx *ctx, int64_t out[6]) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!out) return fail(ctx, TDT_ERR_INVALID_VALUE, "null out pointer");
  Walk W;
  if (int rc = walk_tree(ctx, first_member(ctx), false, W)) return rc;
  out[0] = (int64_t)W.meta.reach; out[1] = (int64_t)W.meta.leaves; out[2] = (int64_t)W.meta.voxels;
  out[3] = (int64_t)W.meta.max_cell; out[4] = (int64_t)W.buffer_cells; out[5] = W.counter;
  return TDT_OK;
}

int tdt_octree_extract(tdt_ctx *ctx, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  tdt_ctx *m = first_member(ctx);
  Walk W;
  if (int rc = walk_tree(ctx, m, voxels_xyzm != nullptr, W)) return rc;
  *n_voxels = (size_t)W.meta.voxels;
  if (W.meta.leaves && W.meta.max_leaf >= 0x7FFFFFFFu) return fail(ctx, TDT_ERR_INVALID_VALUE, "a LEAF value >= 2^31 - 1 does not fit the voxel list");
  if (!voxels_xyzm || W.meta.voxels == 0) return TDT_OK;
  if (capacity < W.meta.voxels)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "capacity " + std::to_string(capacity) + " < " + std::to_string(W.meta.voxels) + " voxels");
  Scratch S;
  int4 *vox = nullptr;
  if (int rc = expand_voxels(ctx, m, W, S, &vox)) return rc;
  TDT_HIP(ctx, hipMemcpyAsync(voxels_xyzm, vox, (size_t)W.meta.voxels * sizeof(int4), hipMemcpyDeviceToHost, m->stream));
  TDT_HIP(ctx, hipStreamSynchronize(m->stream));
  return TDT_OK;
}

int tdt_octree_compact(tdt_ctx *ctx, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  // an edit changes every replica identically (multi_dispatch_compute), so does this; a failure leaves the replicas as they were,
  // and *n_cells too
  return edit_replicas(ctx, false, n_cells, [&](tdt_ctx *m, uint32_t *nc) { return compact_one(ctx, m, nc); });
}

}  // extern "C"
