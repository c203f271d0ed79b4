// Connected components of the tree's voxel set — labels, a component table, and edits of whole objects (include/tdt_rt.h
// tdt_octree_components / tdt_octree_edit_connected / tdt_octree_extract_connected).  On V, the walk of the bound tree
// expanded to its Morton-sorted voxel list (tree_voxels), and its keys:
//
//   hook     one lane per voxel; for each neighbour offset of a fixed half of the set (3 of 6, 13 of 26: the offsets that
//            are lexicographically positive, so each unordered pair is handled once) the neighbour's key, a galloping search
//            from the lane's own index (Morton neighbours are mostly near), and, when found and the match rule allows it, a
//            union.  Lock-free union-find (unionfind_device.hpp, shared with tdt_faces.hip): the larger root is hung under the
//            smaller one by atomicCAS, so the final root of every component is its lowest index whatever the schedule.
//   flatten  a separate launch: root(i), a root flag, exclusive_scan_u32 over the flags -> dense canonical numbers (the
//            Morton order of each component's first voxel).  ONE host synchronisation reads the component count.
//   table    one lane per voxel: its label; labels come in long runs (V is Morton-sorted), so each run of equal labels inside
//            a wave is reduced by a segmented shuffle scan over the 64 lanes and only the run's last lane issues the
//            atomics (size: add; bounding box: min / max).  first and material come from the root lane.
//   select   seeds: one lane per seed, a binary search of its key, the component marked; regions: one lane per voxel runs
//            region_inside, one store per run that touches; then one lane per component applies the size window and invert.
//   apply    region edits' V-only path with the membership selected[label[i]] in place of the shape test (VoxelSelect):
//            op table, scan, gather, rebuild, install.
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "device_scan.hpp"
#include "region_device.hpp"
#include "tdt_internal.hpp"
#include "unionfind_device.hpp"

namespace tdt {

__global__ __launch_bounds__(256) void connect_init_kernel(const int4 *v, uint32_t n, uint32_t *keys, uint32_t *parent) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 p = v[i];
  keys[i] = region_key(p.x, p.y, p.z);
  parent[i] = i;
}

// offsets t = 9 (dx + 1) + 3 (dy + 1) + (dz + 1) above 13 are the lexicographically positive half; 6-connectivity takes
// its faces among them: (0,0,1) = 14, (0,1,0) = 16, (1,0,0) = 22
template <int CONN>
__global__ __launch_bounds__(256) void connect_hook_kernel(const int4 *v, const uint32_t *keys, uint32_t n, int depth, int match,
                                                           uint32_t *parent) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 p = v[i];
  const uint32_t k = keys[i];
  const int N = 1 << depth;
  constexpr int kHalf = CONN == 6 ? 3 : 13;
  for (int h = 0; h < kHalf; h++) {
    const int t = CONN == 6 ? (h == 0 ? 14 : h == 1 ? 16 : 22) : 14 + h;
    const int x = p.x + t / 9 - 1, y = p.y + (t / 3) % 3 - 1, z = p.z + t % 3 - 1;
    if (x < 0 || y < 0 || z < 0 || x >= N || y >= N || z >= N) continue;
    const int j = gallop_find(keys, (int)n, (int)i, k, region_key(x, y, z));
    if (j < 0) continue;
    if (match == TDT_MATCH_MATERIAL && v[j].w != p.w) continue;
    uf_unite(parent, i, (uint32_t)j);
  }
}

// root[i] = the root of i; flag[i] = i is a root; flag[n] = 0 (an exclusive scan over n + 1 leaves the count in [n])
__global__ __launch_bounds__(256) void connect_flatten_kernel(uint32_t *parent, uint32_t n, uint32_t *root, uint32_t *flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  if (i == n) { flag[n] = 0u; return; }
  const uint32_t r = uf_find(parent, i);
  root[i] = r;
  flag[i] = r == i ? 1u : 0u;
}

__global__ __launch_bounds__(256) void connect_table_init_kernel(tdt_component *tab, uint32_t n_comp) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n_comp) return;
  tdt_component e;
  e.first = 0u; e.voxels = 0u;
  e.lo[0] = e.lo[1] = e.lo[2] = INT_MAX;
  e.hi[0] = e.hi[1] = e.hi[2] = INT_MIN;
  e.material = 0; e.pad = 0;
  tab[c] = e;
}

// label[i]: root in, dense label out (each lane reads and writes only its own word); the table by run-aggregated atomics
__global__ __launch_bounds__(256) void connect_table_kernel(const int4 *v, uint32_t n, const uint32_t *excl, uint32_t *label,
                                                            tdt_component *tab) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  const bool live = i < n;
  uint32_t l = 0xFFFFFFFFu;
  int4 p = make_int4(0, 0, 0, 0);
  if (live) {
    const uint32_t r = label[i];
    l = excl[r];
    label[i] = l;
    p = v[i];
    if (r == i) { tab[l].first = i; tab[l].material = p.w; }
  }
  const uint32_t prev = (uint32_t)__shfl_up((int)l, 1, 64);
  const unsigned long long heads = __ballot(lane == 0u || prev != l);
  const uint32_t hs = run_head(heads, lane);
  uint32_t cnt = live ? 1u : 0u;
  int lo0 = p.x, lo1 = p.y, lo2 = p.z, hi0 = p.x, hi1 = p.y, hi2 = p.z;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {                        // segmented inclusive scan: the run's last lane ends with its total
    const uint32_t c_ = (uint32_t)__shfl_up((int)cnt, o, 64);
    const int a0 = __shfl_up(lo0, o, 64), a1 = __shfl_up(lo1, o, 64), a2 = __shfl_up(lo2, o, 64);
    const int b0 = __shfl_up(hi0, o, 64), b1 = __shfl_up(hi1, o, 64), b2 = __shfl_up(hi2, o, 64);
    if (lane >= hs + (uint32_t)o) {
      cnt += c_;
      lo0 = min(lo0, a0); lo1 = min(lo1, a1); lo2 = min(lo2, a2);
      hi0 = max(hi0, b0); hi1 = max(hi1, b1); hi2 = max(hi2, b2);
    }
  }
  const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
  if (live && tail) {
    tdt_component &e = tab[l];
    atomicAdd(&e.voxels, cnt);
    atomicMin(&e.lo[0], lo0); atomicMin(&e.lo[1], lo1); atomicMin(&e.lo[2], lo2);
    atomicMax(&e.hi[0], hi0); atomicMax(&e.hi[1], hi1); atomicMax(&e.hi[2], hi2);
  }
}

// seeds off the grid or on empty voxels match nothing
__global__ __launch_bounds__(256) void connect_seed_kernel(const int4 *seeds, uint32_t n_seeds, const uint32_t *keys, uint32_t n,
                                                           int depth, const uint32_t *label, uint32_t *hit) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_seeds) return;
  const int4 q = seeds[s];
  const int N = 1 << depth;
  if (q.x < 0 || q.y < 0 || q.z < 0 || q.x >= N || q.y >= N || q.z >= N) return;
  const uint32_t k = region_key(q.x, q.y, q.z);
  const uint32_t lo = lower_bound_u32(keys, n, k);
  if (lo < n && keys[lo] == k) hit[label[lo]] = 1u;
}

// a component touches the regions when one of its voxels is inside their union: one store per run of a wave that touches
__global__ __launch_bounds__(256) void connect_touch_kernel(const int4 *v, uint32_t n, const uint32_t *label, const RegionShape *shapes,
                                                            uint32_t n_shapes, uint32_t *touch) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  uint32_t l = 0xFFFFFFFFu;
  bool in = false;
  if (i < n) {
    const int4 p = v[i];
    l = label[i];
    for (uint32_t s = 0; s < n_shapes && !in; s++) in = region_inside(shapes[s], p.x, p.y, p.z);
  }
  const uint32_t prev = (uint32_t)__shfl_up((int)l, 1, 64);
  const unsigned long long heads = __ballot(lane == 0u || prev != l), ins = __ballot(in);
  const unsigned long long from_head = ~((1ull << run_head(heads, lane)) - 1ull), below = (1ull << lane) - 1ull;
  if (in && !(ins & from_head & below)) touch[l] = 1u;     // the run's first lane inside
}

__global__ __launch_bounds__(256) void connect_select_kernel(const tdt_component *tab, uint32_t n_comp, const uint32_t *hit,
                                                             const uint32_t *touch, uint32_t min_voxels, uint32_t max_voxels, int invert,
                                                             uint32_t *selected) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n_comp) return;
  const uint32_t size = tab[c].voxels;
  bool sel = size >= min_voxels && size <= max_voxels;
  if (hit) sel = sel && hit[c] != 0u;
  if (touch) sel = sel && touch[c] != 0u;
  selected[c] = (sel != (invert != 0)) ? 1u : 0u;
}

void connect_flatten(hipStream_t st, uint32_t *parent, uint32_t n, uint32_t *root, uint32_t *flag) {
  hipLaunchKernelGGL(connect_flatten_kernel, dim3(blocks_of((size_t)n + 1)), dim3(256), 0, st, parent, n, root, flag);
}

namespace {

const char *kNoMemory = "out of device memory in the component labelling";

// the components of V on ctx's stream: *label (nv words, in S), *tab (*n_comp entries, in S).  One host synchronisation.
int label_voxels(tdt_ctx *front, tdt_ctx *ctx, const int4 *v, uint32_t nv, int depth, int connectivity, int match, DeviceScratch &S,
                 uint32_t **keys_out, uint32_t **label_out, tdt_component **tab_out, uint32_t *n_comp) {
  *keys_out = nullptr; *label_out = nullptr; *tab_out = nullptr; *n_comp = 0;
  if (nv == 0) return TDT_OK;
  if (nv >= (1u << 31)) return fail(front, TDT_ERR_INVALID_VALUE, "more than 2^31 voxels");
  hipStream_t st = ctx->stream;
  uint32_t *keys = S.get<uint32_t>(nv), *parent = S.get<uint32_t>(nv), *label = S.get<uint32_t>(nv);
  uint32_t *flag = S.get<uint32_t>((size_t)nv + 1), *fscr = S.get<uint32_t>(scan_scratch_words((size_t)nv + 1));
  if (!keys || !parent || !label || !flag || !fscr) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(connect_init_kernel, dim3(blocks_of(nv)), dim3(256), 0, st, v, nv, keys, parent);
  if (connectivity == 6)
    hipLaunchKernelGGL(connect_hook_kernel<6>, dim3(blocks_of(nv)), dim3(256), 0, st, v, (const uint32_t *)keys, nv, depth, match, parent);
  else
    hipLaunchKernelGGL(connect_hook_kernel<26>, dim3(blocks_of(nv)), dim3(256), 0, st, v, (const uint32_t *)keys, nv, depth, match, parent);
  connect_flatten(st, parent, nv, label, flag);
  TDT_HIP(front, exclusive_scan_u32(st, flag, flag, nv + 1u, fscr));
  uint32_t nc = 0;
  if (int rc = read_word(front, st, flag + nv, &nc)) return rc;   // the component count
  tdt_component *tab = S.get<tdt_component>(nc);
  if (!tab) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(connect_table_init_kernel, dim3(blocks_of(nc)), dim3(256), 0, st, tab, nc);
  hipLaunchKernelGGL(connect_table_kernel, dim3(blocks_of(nv)), dim3(256), 0, st, v, nv, (const uint32_t *)flag, label, tab);
  TDT_HIP(front, hipGetLastError());
  *keys_out = keys; *label_out = label; *tab_out = tab; *n_comp = nc;
  return TDT_OK;
}

// what one edit / extract call asks for, checked on the host before anything is queued
// (its host arrays outlive the copies queued from them: region edits drain the stream before they return)
struct Selection final : VoxelSelect {
  tdt_select sel;
  std::vector<int4> seeds;
  std::vector<RegionShape> shapes;

  int run(tdt_ctx *front, tdt_ctx *ctx, const int4 *v, uint32_t nv, int depth, DeviceScratch &S, const uint32_t **label_out,
          const uint32_t **selected_out) override {
    uint32_t *keys = nullptr, *label = nullptr, nc = 0;
    tdt_component *tab = nullptr;
    if (int rc = label_voxels(front, ctx, v, nv, depth, sel.connectivity, sel.match, S, &keys, &label, &tab, &nc)) return rc;
    hipStream_t st = ctx->stream;
    uint32_t *hit = nullptr, *touch = nullptr, *selected = S.get<uint32_t>(nc);
    if (!selected) return fail(front, TDT_ERR_HIP, kNoMemory);
    if (!seeds.empty()) {
      int4 *d_q = S.get<int4>(seeds.size());
      hit = S.get<uint32_t>(nc);
      if (!d_q || !hit) return fail(front, TDT_ERR_HIP, kNoMemory);
      TDT_HIP(front, hipMemsetAsync(hit, 0, (size_t)nc * sizeof(uint32_t), st));
      TDT_HIP(front, hipMemcpyAsync(d_q, seeds.data(), seeds.size() * sizeof(int4), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(connect_seed_kernel, dim3(blocks_of(seeds.size())), dim3(256), 0, st, (const int4 *)d_q, (uint32_t)seeds.size(),
                         (const uint32_t *)keys, nv, depth, (const uint32_t *)label, hit);
    }
    if (!shapes.empty()) {
      RegionShape *d_shapes = nullptr;
      touch = S.get<uint32_t>(nc);
      if (!touch) return fail(front, TDT_ERR_HIP, kNoMemory);
      TDT_HIP(front, hipMemsetAsync(touch, 0, (size_t)nc * sizeof(uint32_t), st));
      if (int rc = upload_shapes(front, st, S, shapes.data(), shapes.size(), kNoMemory, &d_shapes)) return rc;
      hipLaunchKernelGGL(connect_touch_kernel, dim3(blocks_of(nv)), dim3(256), 0, st, v, nv, (const uint32_t *)label,
                         (const RegionShape *)d_shapes, (uint32_t)shapes.size(), touch);
    }
    hipLaunchKernelGGL(connect_select_kernel, dim3(blocks_of(nc)), dim3(256), 0, st, (const tdt_component *)tab, nc, (const uint32_t *)hit,
                       (const uint32_t *)touch, sel.min_voxels, sel.max_voxels, sel.invert, selected);
    TDT_HIP(front, hipGetLastError());
    *label_out = label; *selected_out = selected;
    return TDT_OK;
  }
};

int check_kind(tdt_ctx *ctx, int connectivity, int match) {
  if (connectivity != 6 && connectivity != 26) return fail(ctx, TDT_ERR_INVALID_VALUE, "connectivity must be 6 or 26");
  if (match != TDT_MATCH_ANY && match != TDT_MATCH_MATERIAL) return fail(ctx, TDT_ERR_INVALID_VALUE, "match must be a TDT_MATCH_* value");
  return TDT_OK;
}

int make_selection(tdt_ctx *ctx, const tdt_select *sel, const int32_t *seeds, size_t n_seeds, const tdt_region *regions, size_t n_regions,
                   Selection &out) {
  if (!sel) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_select pointer");
  if (int rc = check_kind(ctx, sel->connectivity, sel->match)) return rc;
  if (sel->invert != 0 && sel->invert != 1) return fail(ctx, TDT_ERR_INVALID_VALUE, "invert must be 0 or 1");
  if (sel->min_voxels > sel->max_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "min_voxels > max_voxels");
  if (n_seeds && !seeds) return fail(ctx, TDT_ERR_INVALID_VALUE, "null seed list");
  if (n_seeds >= (1ull << 31)) return fail(ctx, TDT_ERR_INVALID_VALUE, "more than 2^31 seeds");
  if (int rc = region_shapes(ctx, regions, n_regions, &out.shapes)) return rc;
  out.sel = *sel;
  out.seeds.resize(n_seeds);
  for (size_t s = 0; s < n_seeds; s++) out.seeds[s] = make_int4(seeds[3 * s], seeds[3 * s + 1], seeds[3 * s + 2], 0);
  return TDT_OK;
}

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_components(tdt_ctx *ctx, int connectivity, int match, uint32_t *labels, size_t labels_capacity, size_t *n_voxels,
                          tdt_component *components, size_t capacity, size_t *n_components) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels || !n_components) return fail(ctx, TDT_ERR_INVALID_VALUE, "null count pointer");
  *n_voxels = 0; *n_components = 0;
  if (int rc = check_kind(ctx, connectivity, match)) return rc;
  tdt_ctx *m = first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  DeviceScratch S;
  int4 *v = nullptr;
  uint32_t nv = 0, nc = 0, *keys = nullptr, *label = nullptr;
  int depth = 0;
  if (int rc = tree_voxels(ctx, m, 0x7FFFFFFFu, S, &v, &nv, &depth)) return rc;
  tdt_component *tab = nullptr;
  if (int rc = label_voxels(ctx, m, v, nv, depth, connectivity, match, S, &keys, &label, &tab, &nc)) return rc;
  *n_voxels = nv; *n_components = nc;
  if (labels && labels_capacity < nv)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "labels capacity " + std::to_string(labels_capacity) + " < " + std::to_string(nv) + " voxels");
  if (components && capacity < nc)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "capacity " + std::to_string(capacity) + " < " + std::to_string(nc) + " components");
  hipStream_t st = m->stream;
  if (labels && nv) TDT_HIP(ctx, hipMemcpyAsync(labels, label, (size_t)nv * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (components && nc) TDT_HIP(ctx, hipMemcpyAsync(components, tab, (size_t)nc * sizeof(tdt_component), hipMemcpyDeviceToHost, st));
  TDT_HIP(ctx, hipStreamSynchronize(st));
  return TDT_OK;
}

int tdt_octree_edit_connected(tdt_ctx *ctx, int op, const tdt_select *sel, const int32_t *seeds_xyz, size_t n_seeds,
                              const tdt_region *regions, size_t n_regions, int32_t material, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (op != TDT_REGION_PAINT && op != TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be TDT_REGION_PAINT or TDT_REGION_CLEAR");
  if (material < 0 || material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be 0..253");
  Selection S;
  if (int rc = make_selection(ctx, sel, seeds_xyz, n_seeds, regions, n_regions, S)) return rc;
  return region_edit_selected(ctx, op, material, S, n_cells);
}

int tdt_octree_extract_connected(tdt_ctx *ctx, const tdt_select *sel, const int32_t *seeds_xyz, size_t n_seeds,
                                 const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm, size_t capacity,
                                 size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  Selection S;
  if (int rc = make_selection(ctx, sel, seeds_xyz, n_seeds, regions, n_regions, S)) return rc;
  return region_extract_selected(ctx, S, voxels_xyzm, capacity, n_voxels);
}

}  // extern "C"
