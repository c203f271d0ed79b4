// Face tools (include/tdt_rt.h tdt_octree_face_regions / tdt_octree_extract_faces / tdt_octree_edit_faces): the tree's exposed
// faces labelled into coplanar face regions — the 2-D analogue of tdt_connect.hip's components — and the regions under a list of
// seeds swept along their normal into a Morton-sorted voxel list that the region edits install.
//
//   faces    surface_face_list (surface_device.hpp; tdt_surface.hip owns and launches it): walk, keys, exposed-face probe under
//            the mask, scan, emit, per-segment sort.  F = six segments, one per direction, of (w << 20 | u << 10 | v,
//            u << 8 | material + 1) sorted by key: the face list of tdt_octree_extract_surface(merge = 0, by_material = 1).
//   hook     one lane per face j.  Inside a segment equal w are contiguous and a row (w, u) is a run of ascending v, so of the
//            positive half of the neighbours (u, v + 1) is lane j + 1 iff its key is key + 1 and v != 1023 (at depth 10 key + 1
//            carries into u), and (u + 1, v - 1), (u + 1, v), (u + 1, v + 1) have the consecutive keys key + 1023 .. key + 1025:
//            ONE bounded galloping search forward for the first of them, never across the segment's end, then up to two steps.
//            u == 1023 has no row above (key + 1024 would carry into w).  Union-find: unionfind_device.hpp, tdt_connect.hip's.
//            Pre-merge (the default): faces_init_kernel hangs every face under the first lane of its run along v inside its
//            wave (a ballot, no atomics), so the hook unites (j, j + 1) only across a wave's end, and lane j skips the union
//            with (u + 1, v) when lane j - 1 of the same run reaches (u + 1, v - 1) of the same run: one union per pair of
//            touching runs instead of one per pair of touching faces.  Measured against the plain hook (tdt_debug_faces_premerge,
//            tools/faces_time.py): both label alike.                            faces_init_kernel, faces_hook_kernel
//   flatten  connect_flatten (tdt_connect.hip), exclusive_scan_u32 over the root flags: dense numbers in the order of each
//            region's first face in F.  ONE host synchronisation reads the region count.
//   table    one lane per face; labels come in runs along v, reduced inside the wave by connect's segmented shuffle scan, the
//            run's last lane issuing the atomics (size: add; (u, v) box: min / max).  first, face, w and material come from the
//            root lane.                                                                                      faces_table_kernel
//   seeds    one lane per seed: a binary search for (w, u, v) inside segment f, then one flag per region.     faces_seed_kernel
//   columns  one lane per face of a flagged region counts its column (the clipped length; block = 1: a gallop_find in V's keys per
//            step) and the wave adds its total to a 64-bit word the host checks against the cap before anything is sized by it
//            (ONE synchronisation); scan; one lane per (face, k) pair finds its face by a binary search of the scan and writes
//            (Morton key, material): pairs in (face order, k) order, stores coalesced.      faces_count_kernel, faces_emit_kernel
//   unique   the stable sort_pairs_u32 keeps that order inside every run of equal keys and voxlist_last_flags keeps the last;
//            scan; {x, y, z, m} per kept key.  ONE synchronisation reads the voxel count.                     faces_list_kernel
//
// Host synchronisations: tdt_octree_face_regions: tree_voxels' own, the segment bounds, the region count, the copy out.  A column
// list (one per replica of an edit): those first three, the pair total and the voxel count; then what region_edit_source /
// region_intersect_source / region_extract_source add.
#include <climits>
#include <string>
#include <vector>

#include "device_scan.hpp"
#include "region_device.hpp"
#include "surface_device.hpp"
#include "tdt_internal.hpp"
#include "unionfind_device.hpp"

namespace tdt {

constexpr uint32_t kFaceSeeds = 1u << 20;
constexpr unsigned long long kFacePairs = kVoxelListCap;     // (face, voxel) pairs of the columns

__device__ __forceinline__ bool faces_same_material(int match, uint32_t a, uint32_t b) {
  return match == TDT_MATCH_ANY || ((a ^ b) & 255u) == 0u;
}

// is face j (key, val) the successor along v of face j - 1, inside its wave and its segment [lo, ..)?
__device__ __forceinline__ bool faces_joined(const uint32_t *fk, const uint32_t *fv, uint32_t j, uint32_t lo, uint32_t key, uint32_t val, int match) {
  return (j & 63u) != 0u && j > lo && (key & 1023u) != 0u && fk[j - 1u] + 1u == key && faces_same_material(match, fv[j - 1u], val);
}

// parent[j] = j, or with the pre-merge the first face of j's run along v inside its wave
template <bool PREMERGE>
__global__ __launch_bounds__(256) void faces_init_kernel(const uint32_t *fk, const uint32_t *fv, uint32_t n, SurfaceSegs segs, int match,
                                                         uint32_t *parent) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  const bool live = j < n;
  if (!PREMERGE) { if (live) parent[j] = j; return; }
  bool head = true;
  if (live) head = !faces_joined(fk, fv, j, surface_seg_start(segs, j), fk[j], fv[j], match);
  const unsigned long long heads = __ballot(head);
  if (live) parent[j] = j - (lane - run_head(heads, lane));
}

// the first index in (j, hi) whose key is >= t, or hi: a gallop from j (fk[j] < t), then a binary search
__device__ __forceinline__ uint32_t faces_gallop_lower(const uint32_t *fk, uint32_t j, uint32_t hi, uint32_t t) {
  uint32_t a = j, b = hi;                                  // fk[a] < t <= fk[b] (b = hi: past the end)
  for (uint32_t step = 1; step < hi - j; step <<= 1) {
    const uint32_t i = j + step;
    if (fk[i] >= t) { b = i; break; }
    a = i;
  }
  while (b - a > 1u) { const uint32_t mid = a + ((b - a) >> 1); if (fk[mid] < t) a = mid; else b = mid; }
  return b;
}

template <int CONN, bool PREMERGE>
__global__ __launch_bounds__(256) void faces_hook_kernel(const uint32_t *fk, const uint32_t *fv, uint32_t n, SurfaceSegs segs, int match,
                                                         uint32_t *parent) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t lo = surface_seg_start(segs, j), hi = surface_seg_end(segs, j);
  const uint32_t key = fk[j], val = fv[j];
  const uint32_t u = (key >> 10) & 1023u, v = key & 1023u;
  // (u, v + 1): inside a wave the pre-merge has joined it already
  if ((!PREMERGE || (j & 63u) == 63u) && v != 1023u && j + 1u < hi && fk[j + 1u] == key + 1u && faces_same_material(match, fv[j + 1u], val))
    uf_unite(parent, j, j + 1u);
  if (u == 1023u) return;
  const bool below = CONN == 8 && v != 0u;                 // (u + 1, v - 1) exists on the grid
  uint32_t p = faces_gallop_lower(fk, j, hi, key + (below ? 1023u : 1024u));
  if (below && p < hi && fk[p] == key + 1023u) {
    if (faces_same_material(match, fv[p], val)) uf_unite(parent, j, p);
    p++;
  }
  if (p < hi && fk[p] == key + 1024u) {                    // (u + 1, v)
    if (faces_same_material(match, fv[p], val)) {
      // lane j - 1, joined to j, unites (or skips in turn) with p - 1 = (u + 1, v - 1), joined to p: the two runs are one already
      const bool skip = PREMERGE && faces_joined(fk, fv, j, lo, key, val, match) && faces_joined(fk, fv, p, lo, key + 1024u, fv[p], match);
      if (!skip) uf_unite(parent, j, p);
    }
    p++;
  }
  if (CONN == 8 && v != 1023u && p < hi && fk[p] == key + 1025u && faces_same_material(match, fv[p], val)) uf_unite(parent, j, p);
}

__global__ __launch_bounds__(256) void faces_table_init_kernel(tdt_face_region *tab, uint32_t n_regions) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n_regions) return;
  tdt_face_region e;
  e.first = 0u; e.faces = 0u; e.face = 0; e.w = 0;
  e.lo[0] = e.lo[1] = INT_MAX;
  e.hi[0] = e.hi[1] = INT_MIN;
  e.material = 0; e.pad = 0;
  tab[c] = e;
}

// label[j]: root in, dense label out (each lane reads and writes only its own word); the table by run-aggregated atomics
__global__ __launch_bounds__(256) void faces_table_kernel(const uint32_t *fk, const uint32_t *fv, uint32_t n, SurfaceSegs segs, const uint32_t *excl,
                                                          uint32_t *label, tdt_face_region *tab) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  const bool live = j < n;
  uint32_t l = 0xFFFFFFFFu;
  int pu = 0, pv = 0;
  if (live) {
    const uint32_t r = label[j], key = fk[j];
    l = excl[r];
    label[j] = l;
    pu = (int)((key >> 10) & 1023u); pv = (int)(key & 1023u);
    if (r == j) {
      tdt_face_region &e = tab[l];
      e.first = j; e.face = surface_seg_of(segs, j); e.w = (int)(key >> 20); e.material = (int)(fv[j] & 255u);
    }
  }
  const uint32_t prev = (uint32_t)__shfl_up((int)l, 1, 64);
  const unsigned long long heads = __ballot(lane == 0u || prev != l);
  const uint32_t hs = run_head(heads, lane);
  uint32_t cnt = live ? 1u : 0u;
  int lo0 = pu, lo1 = pv, hi0 = pu, hi1 = pv;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {                        // segmented inclusive scan: the run's last lane ends with its total
    const uint32_t c_ = (uint32_t)__shfl_up((int)cnt, o, 64);
    const int a0 = __shfl_up(lo0, o, 64), a1 = __shfl_up(lo1, o, 64);
    const int b0 = __shfl_up(hi0, o, 64), b1 = __shfl_up(hi1, o, 64);
    if (lane >= hs + (uint32_t)o) {
      cnt += c_;
      lo0 = min(lo0, a0); lo1 = min(lo1, a1);
      hi0 = max(hi0, b0); hi1 = max(hi1, b1);
    }
  }
  const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
  if (live && tail) {
    tdt_face_region &e = tab[l];
    atomicAdd(&e.faces, cnt);
    atomicMin(&e.lo[0], lo0); atomicMin(&e.lo[1], lo1);
    atomicMax(&e.hi[0], hi0); atomicMax(&e.hi[1], hi1);
  }
}

// seeds {x, y, z, f}, f 0..5 (the host has checked it); a seed that is no face of F flags nothing
__global__ __launch_bounds__(256) void faces_seed_kernel(const int4 *seeds, uint32_t n_seeds, const uint32_t *fk, SurfaceSegs segs, int depth,
                                                         const uint32_t *label, uint32_t *hit) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_seeds) return;
  const int4 q = seeds[s];
  const int N = 1 << depth;
  if (q.x < 0 || q.y < 0 || q.z < 0 || q.x >= N || q.y >= N || q.z >= N) return;
  const int a = q.w >> 1;
  const uint32_t w = (uint32_t)(a == 0 ? q.x : a == 1 ? q.y : q.z), u = (uint32_t)(a == 0 ? q.y : a == 1 ? q.z : q.x),
                 v = (uint32_t)(a == 0 ? q.z : a == 1 ? q.x : q.y);
  uint32_t lo = segs.at[0], hi = segs.at[1];
#pragma unroll
  for (int f = 1; f < 6; f++) if (q.w == f) { lo = segs.at[f]; hi = segs.at[f + 1]; }
  const uint32_t key = w << 20 | u << 10 | v;
  const uint32_t i = lo + lower_bound_u32(fk + lo, hi - lo, key);
  if (i < hi && fk[i] == key) hit[label[i]] = 1u;
}

// the voxel k steps from (w, u, v) along axis a (k may be negative)
__device__ __forceinline__ uint32_t faces_column_key(int a, int w, int u, int v, int k) {
  const int c = w + k;
  return a == 0 ? region_key(c, u, v) : a == 1 ? region_key(v, c, u) : region_key(u, v, c);
}

// cnt[j] = the voxels of face j's column (0: its region is not selected), cnt[n] = 0; *total += them
__global__ __launch_bounds__(256) void faces_count_kernel(const uint32_t *fk, const uint32_t *label, const uint32_t *hit, uint32_t n, SurfaceSegs segs,
                                                          const uint32_t *keys, uint32_t nv, int depth, int distance, int block, uint32_t *cnt,
                                                          unsigned long long *total) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  uint32_t c = 0;
  if (j < n && hit[label[j]]) {
    const int f = surface_seg_of(segs, j), a = f >> 1, out = (f & 1) ? 1 : -1, N = 1 << depth;
    const uint32_t key = fk[j];
    const int w = (int)(key >> 20), u = (int)((key >> 10) & 1023u), v = (int)(key & 1023u);
    const int step = distance > 0 ? out : -out, len = distance > 0 ? distance : -distance;
    const int first = distance > 0 ? w + out : w;                        // the column: first + step * t, t = 0 .. len - 1
    const int room = step > 0 ? N - first : first + 1;                   // of them inside the grid
    c = (uint32_t)(room < 0 ? 0 : room < len ? room : len);
    if (block && c) {
      uint32_t k = faces_column_key(a, w, u, v, 0);
      int i = (int)lower_bound_u32(keys, nv, k);                         // the owner: a voxel of V
      for (uint32_t t = distance > 0 ? 0u : 1u; t < c; t++) {
        const uint32_t kn = faces_column_key(a, first, u, v, step * (int)t);
        const int g = gallop_find(keys, (int)nv, i, k, kn);
        if (distance > 0 ? g >= 0 : g < 0) { c = t; break; }             // a pull ends at an obstacle, a push at the air
        if (g >= 0) { i = g; k = kn; }
      }
    }
  }
  if (j <= n) cnt[j] = c;
  uint32_t sum = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o, 64);
  if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(total, (unsigned long long)sum);
}

// pair g = voxel t = g - excl[j] of the column of face j, the last face whose first pair is <= g (a face without pairs shares
// its successor's first pair, so it is never the last)
__global__ __launch_bounds__(256) void faces_emit_kernel(const uint32_t *fk, const uint32_t *fv, uint32_t n, SurfaceSegs segs, const uint32_t *excl,
                                                         uint32_t n_pairs, int distance, int material1, uint32_t *ok, uint32_t *ov) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_pairs) return;
  const uint32_t j = upper_bound_u32(excl, n + 1u, g) - 1u;
  const int t = (int)(g - excl[j]);
  const int f = surface_seg_of(segs, j), a = f >> 1, out = (f & 1) ? 1 : -1;
  const uint32_t key = fk[j];
  const int w = (int)(key >> 20), u = (int)((key >> 10) & 1023u), v = (int)(key & 1023u);
  ok[g] = faces_column_key(a, w, u, v, distance > 0 ? out * (1 + t) : -out * t);
  ov[g] = material1 ? (uint32_t)material1 : (fv[j] & 255u);
}

__global__ __launch_bounds__(256) void faces_list_kernel(const uint32_t *keys, const uint32_t *vals, uint32_t n, const uint32_t *excl, int4 *out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || excl[i + 1u] == excl[i]) return;
  out[excl[i]] = region_voxel(keys[i], (int)vals[i]);
}

namespace {

const char *kNoMemory = "out of device memory in the face tools";

struct FaceLabels {
  SurfaceFaces L;
  uint32_t *label = nullptr;       // L.nf words
  tdt_face_region *tab = nullptr;  // n_regions entries
  uint32_t n_regions = 0;
};

// F and its face regions on ctx's stream, everything in S
int label_faces(tdt_ctx *front, tdt_ctx *ctx, int connectivity, int match, const std::vector<RegionShape> &shapes, DeviceScratch &S, FaceLabels &R) {
  R = FaceLabels{};
  if (int rc = surface_face_list(front, ctx, shapes, 1, 1, S, R.L)) return rc;
  const uint32_t nf = R.L.nf;
  if (nf == 0) return TDT_OK;
  hipStream_t st = ctx->stream;
  const uint32_t *fk = R.L.fk, *fv = R.L.fv;
  const SurfaceSegs segs = R.L.segs;
  uint32_t *parent = R.L.fk_alt, *label = R.L.fv_alt;        // the sort's second pair is free now
  uint32_t *flag = S.get<uint32_t>((size_t)nf + 1), *fscr = S.get<uint32_t>(scan_scratch_words((size_t)nf + 1));
  if (!flag || !fscr) return fail(front, TDT_ERR_HIP, kNoMemory);
  const dim3 grid(blocks_of(nf)), block(256);
  if (front->faces_premerge) {
    hipLaunchKernelGGL(faces_init_kernel<true>, grid, block, 0, st, fk, fv, nf, segs, match, parent);
    if (connectivity == 4) hipLaunchKernelGGL((faces_hook_kernel<4, true>), grid, block, 0, st, fk, fv, nf, segs, match, parent);
    else hipLaunchKernelGGL((faces_hook_kernel<8, true>), grid, block, 0, st, fk, fv, nf, segs, match, parent);
  } else {
    hipLaunchKernelGGL(faces_init_kernel<false>, grid, block, 0, st, fk, fv, nf, segs, match, parent);
    if (connectivity == 4) hipLaunchKernelGGL((faces_hook_kernel<4, false>), grid, block, 0, st, fk, fv, nf, segs, match, parent);
    else hipLaunchKernelGGL((faces_hook_kernel<8, false>), grid, block, 0, st, fk, fv, nf, segs, match, parent);
  }
  connect_flatten(st, parent, nf, label, flag);
  TDT_HIP(front, exclusive_scan_u32(st, flag, flag, nf + 1u, fscr));
  uint32_t nr = 0;
  if (int rc = read_word(front, st, flag + nf, &nr)) return rc;   // the region count
  tdt_face_region *tab = S.get<tdt_face_region>(nr);
  if (!tab) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(faces_table_init_kernel, dim3(blocks_of(nr)), block, 0, st, tab, nr);
  hipLaunchKernelGGL(faces_table_kernel, grid, block, 0, st, fk, fv, nf, segs, (const uint32_t *)flag, label, tab);
  TDT_HIP(front, hipGetLastError());
  R.label = label; R.tab = tab; R.n_regions = nr;
  return TDT_OK;
}

int check_kind(tdt_ctx *ctx, int connectivity, int match) {
  if (connectivity != 4 && connectivity != 8) return fail(ctx, TDT_ERR_INVALID_VALUE, "connectivity must be 4 or 8");
  if (match != TDT_MATCH_ANY && match != TDT_MATCH_MATERIAL) return fail(ctx, TDT_ERR_INVALID_VALUE, "match must be a TDT_MATCH_* value");
  return TDT_OK;
}

// what one edit / extract call asks for, checked on the host before anything is queued
struct FacesSource final : VoxelSource {
  tdt_faces opt;
  std::vector<int4> seeds;
  std::vector<RegionShape> shapes;

  int run(tdt_ctx *front, tdt_ctx *ctx, int /*depth*/, DeviceScratch &S, const int4 **out, uint32_t *n) override {
    *out = nullptr; *n = 0;
    if (seeds.empty() || opt.distance == 0) return TDT_OK;
    FaceLabels R;
    if (int rc = label_faces(front, ctx, opt.connectivity, opt.match, shapes, S, R)) return rc;
    const uint32_t nf = R.L.nf, nr = R.n_regions;
    if (nf == 0) return TDT_OK;
    hipStream_t st = ctx->stream;
    const SurfaceSegs segs = R.L.segs;
    // ---- seeds ----
    int4 *d_q = S.get<int4>(seeds.size());
    uint32_t *hit = S.get<uint32_t>(nr), *cnt = S.get<uint32_t>((size_t)nf + 1), *cscr = S.get<uint32_t>(scan_scratch_words((size_t)nf + 1));
    unsigned long long *d_total = S.get<unsigned long long>(1);
    if (!d_q || !hit || !cnt || !cscr || !d_total) return fail(front, TDT_ERR_HIP, kNoMemory);
    TDT_HIP(front, hipMemsetAsync(hit, 0, (size_t)nr * sizeof(uint32_t), st));
    TDT_HIP(front, hipMemsetAsync(d_total, 0, sizeof *d_total, st));
    TDT_HIP(front, hipMemcpyAsync(d_q, seeds.data(), seeds.size() * sizeof(int4), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(faces_seed_kernel, dim3(blocks_of(seeds.size())), dim3(256), 0, st, (const int4 *)d_q, (uint32_t)seeds.size(),
                       (const uint32_t *)R.L.fk, segs, R.L.depth, (const uint32_t *)R.label, hit);
    // ---- columns: count, then emit ----
    hipLaunchKernelGGL(faces_count_kernel, dim3(blocks_of((size_t)nf + 1)), dim3(256), 0, st, (const uint32_t *)R.L.fk, (const uint32_t *)R.label,
                       (const uint32_t *)hit, nf, segs, (const uint32_t *)R.L.keys, R.L.nv, R.L.depth, opt.distance, opt.block, cnt, d_total);
    TDT_HIP(front, hipGetLastError());
    unsigned long long pairs = 0;
    TDT_HIP(front, hipMemcpyAsync(&pairs, d_total, sizeof pairs, hipMemcpyDeviceToHost, st));
    TDT_HIP(front, hipStreamSynchronize(st));                // the (face, voxel) pairs
    if (pairs > kFacePairs)
      return fail(front, TDT_ERR_INVALID_VALUE, "the columns hold " + std::to_string(pairs) + " (face, voxel) pairs (more than 2^26)");
    if (pairs == 0) return TDT_OK;
    const uint32_t nk = (uint32_t)pairs;
    uint32_t *k0 = S.get<uint32_t>(nk), *v0 = S.get<uint32_t>(nk), *k1 = S.get<uint32_t>(nk), *v1 = S.get<uint32_t>(nk);
    uint32_t *hist = S.get<uint32_t>(sort_hist_words(nk)), *hscr = S.get<uint32_t>(sort_scratch_words(nk));
    uint32_t *last = S.get<uint32_t>((size_t)nk + 1), *lscr = S.get<uint32_t>(scan_scratch_words((size_t)nk + 1));
    int4 *vox = S.get<int4>(nk);
    if (!k0 || !v0 || !k1 || !v1 || !hist || !hscr || !last || !lscr || !vox) return fail(front, TDT_ERR_HIP, kNoMemory);
    TDT_HIP(front, exclusive_scan_u32(st, cnt, cnt, nf + 1u, cscr));
    hipLaunchKernelGGL(faces_emit_kernel, dim3(blocks_of(nk)), dim3(256), 0, st, (const uint32_t *)R.L.fk, (const uint32_t *)R.L.fv, nf, segs,
                       (const uint32_t *)cnt, nk, opt.distance, opt.material + 1, k0, v0);
    // ---- sort, last of each run, the list ----
    uint32_t *k = k0, *v = v0;
    TDT_HIP(front, sort_pairs_u32(st, k, v, k1, v1, nk, hist, hscr));
    voxlist_last_flags(st, k, nk, last);
    TDT_HIP(front, exclusive_scan_u32(st, last, last, nk + 1u, lscr));
    hipLaunchKernelGGL(faces_list_kernel, dim3(blocks_of(nk)), dim3(256), 0, st, (const uint32_t *)k, (const uint32_t *)v, nk, (const uint32_t *)last, vox);
    TDT_HIP(front, hipGetLastError());
    uint32_t nu = 0;
    if (int rc = read_word(front, st, last + nk, &nu)) return rc;   // the voxel count
    *out = vox; *n = nu;
    return TDT_OK;
  }
};

int make_source(tdt_ctx *ctx, const tdt_faces *f, const int32_t *seeds, size_t n_seeds, const tdt_region *regions, size_t n_regions, FacesSource &out) {
  if (!f) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_faces pointer");
  if (int rc = check_kind(ctx, f->connectivity, f->match)) return rc;
  if (f->distance < -TDT_FACES_DISTANCE_MAX || f->distance > TDT_FACES_DISTANCE_MAX) return fail(ctx, TDT_ERR_INVALID_VALUE, "distance must be -1023..1023");
  if (f->block != 0 && f->block != 1) return fail(ctx, TDT_ERR_INVALID_VALUE, "block must be 0 or 1");
  if (f->material < -1 || f->material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be -1..253");
  if (f->pad != 0) return fail(ctx, TDT_ERR_INVALID_VALUE, "pad must be 0");
  if (n_seeds && !seeds) return fail(ctx, TDT_ERR_INVALID_VALUE, "null seed list");
  if (n_seeds > kFaceSeeds) return fail(ctx, TDT_ERR_INVALID_VALUE, "more than 2^20 seeds");
  for (size_t s = 0; s < n_seeds; s++)
    if (seeds[4 * s + 3] < 0 || seeds[4 * s + 3] > 5)
      return fail(ctx, TDT_ERR_INVALID_VALUE, "seed " + std::to_string(s) + ": face " + std::to_string(seeds[4 * s + 3]) + " is not 0..5");
  if (int rc = region_shapes(ctx, regions, n_regions, &out.shapes)) return rc;
  out.opt = *f;
  out.seeds.resize(n_seeds);
  for (size_t s = 0; s < n_seeds; s++) out.seeds[s] = make_int4(seeds[4 * s], seeds[4 * s + 1], seeds[4 * s + 2], seeds[4 * s + 3]);
  return TDT_OK;
}

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_face_regions(tdt_ctx *ctx, int connectivity, int match, const tdt_region *regions, size_t n_regions, tdt_quad *faces,
                            uint32_t *labels, size_t faces_capacity, size_t *n_faces, tdt_face_region *table, size_t capacity,
                            size_t *n_face_regions) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_faces || !n_face_regions) return fail(ctx, TDT_ERR_INVALID_VALUE, "null count pointer");
  *n_faces = 0; *n_face_regions = 0;
  if (int rc = check_kind(ctx, connectivity, match)) return rc;
  std::vector<RegionShape> shapes;
  if (int rc = region_shapes(ctx, regions, n_regions, &shapes)) return rc;
  tdt_ctx *m = first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  DeviceScratch S;
  Drain drain{m->stream};                                // before S is freed
  FaceLabels R;
  if (int rc = label_faces(ctx, m, connectivity, match, shapes, S, R)) return rc;
  const uint32_t nf = R.L.nf, nr = R.n_regions;
  *n_faces = nf; *n_face_regions = nr;
  if ((faces || labels) && faces_capacity < nf)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "faces capacity " + std::to_string(faces_capacity) + " < " + std::to_string(nf) + " faces");
  if (table && capacity < nr)
    return fail(ctx, TDT_ERR_INVALID_VALUE, "capacity " + std::to_string(capacity) + " < " + std::to_string(nr) + " face regions");
  if (nf == 0) return TDT_OK;
  hipStream_t st = m->stream;
  if (faces) {
    int4 *d_quads = S.get<int4>(2 * (size_t)nf);
    if (!d_quads) return fail(ctx, TDT_ERR_HIP, kNoMemory);
    surface_unit_quads(st, R.L.fk, R.L.fv, nf, R.L.segs, d_quads);
    TDT_HIP(ctx, hipGetLastError());
    TDT_HIP(ctx, hipMemcpyAsync(faces, d_quads, (size_t)nf * sizeof(tdt_quad), hipMemcpyDeviceToHost, st));
  }
  if (labels) TDT_HIP(ctx, hipMemcpyAsync(labels, R.label, (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (table) TDT_HIP(ctx, hipMemcpyAsync(table, R.tab, (size_t)nr * sizeof(tdt_face_region), hipMemcpyDeviceToHost, st));
  TDT_HIP(ctx, hipStreamSynchronize(st));
  return TDT_OK;
}

int tdt_octree_extract_faces(tdt_ctx *ctx, const tdt_faces *faces, const int32_t *seeds_xyzf, size_t n_seeds, const tdt_region *regions,
                             size_t n_regions, int what, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  if (what != TDT_FACES_COLUMNS && what != TDT_FACES_TREE) return fail(ctx, TDT_ERR_INVALID_VALUE, "what must be a TDT_FACES_* value");
  FacesSource src;
  if (int rc = make_source(ctx, faces, seeds_xyzf, n_seeds, regions, n_regions, src)) return rc;
  if (what == TDT_FACES_TREE) return region_intersect_source(ctx, src, voxels_xyzm, capacity, n_voxels);
  int depth = 0;
  if (int rc = walk_inputs(ctx, first_member(ctx), &depth)) return rc;
  return region_extract_source(ctx, src, depth, voxels_xyzm, capacity, n_voxels);
}

int tdt_octree_edit_faces(tdt_ctx *ctx, int op, const tdt_faces *faces, const int32_t *seeds_xyzf, size_t n_seeds,
                          const tdt_region *regions, size_t n_regions, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (op < TDT_REGION_SET || op > TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  FacesSource src;
  if (int rc = make_source(ctx, faces, seeds_xyzf, n_seeds, regions, n_regions, src)) return rc;
  return region_edit_source(ctx, op, src, n_cells);
}

int tdt_debug_faces_premerge(tdt_ctx *ctx, int on) {
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  ctx->faces_premerge = on ? 1 : 0;
  return TDT_OK;
}

}  // extern "C"
