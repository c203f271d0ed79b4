// Surface extraction — the tree's exposed faces as merged quads (include/tdt_rt.h tdt_octree_extract_surface).  Works on the
// Morton-sorted voxel list (tree_voxels) and its keys, like voxel morphology; the tree is only read.
//
//   probe    one lane per voxel: the six face-neighbour keys looked up with gallop_find.  One word per voxel: bit f set = face f
//            is exposed (the neighbour is absent or outside the grid) and the voxel is inside the mask.  The same launch writes
//            six 0 / 1 count arrays of nv + 1 words laid end to end (each ends in a 0), so ONE exclusive_scan_u32 over all
//            6 (nv + 1) words numbers the faces direction by direction: the faces of direction f are the SEGMENT
//            [excl[f (nv + 1)], excl[(f + 1) (nv + 1)]) of one array.  Synchronisation: the seven segment bounds.
//   emit     lane i writes each of its exposed faces at its scanned position, no atomics: (w << 20 | v << 10 | u, carried
//            material) — w is the voxel's OWN coordinate along the axis (10 bits; the plane w + s reaches 1024 at depth 10 and is
//            formed only when a quad is written).  merge = 0 emits (w << 20 | u << 10 | v, u << 8 | material) instead: that is
//            already the order and the payload of the last stage, and every face is its own quad.
//   sort     sort_pairs_u32 per segment (six sorts; the key has no room for the direction: 30 + 3 bits).
//   runs     head flag over the whole array: a segment's first item, previous key + 1 != key, u == 0, or another material.
//            exclusive_scan_u32 numbers the runs across all segments; a head writes its position into start[run], the lane past
//            the end writes the sentinel start[runs] = faces, so run r spans start[r] .. start[r + 1] and needs no walk.
//            Synchronisation: the seven run-segment bounds (they size the second sorts).
//   stacks   one lane per run emits (w << 20 | u0 << 10 | v, u1 << 8 | material); sort per segment; the SAME head-flag kernel
//            (previous key + 1 != key or v == 0: another (w, u0) or a gap in v; another value: another u1 or material), scan,
//            start positions.  Synchronisation: the seven quad-segment bounds (their last is the count the caller gets).
//   quads    one lane per quad reads its first run and its length and writes the 32-byte tdt_quad with two 16-byte stores.
//            Segments are in face order and each is sorted by (w, u0, v0): the array is the result as it stands.
//
// The first three stages — walk, keys, probe, scan, emit, sort — are surface_face_list (surface_device.hpp): the ONE definition of the face
// list, which tdt_faces.hip labels into face regions; surface_unit_quads is the last stage over a merge = 0 list for that unit.
//
// Host synchronisations per call: tree_voxels' own, then 1 (merge = 0) or 3 (merge = 1) for the lengths above, then the copy of
// the quads.  The six directions share every launch except the sorts; whether fusing the sorts too (a 64-bit key) or running
// six independent passes would be faster is NOT measured.  Measured (tools/surface_time.py): on large trees the walk
// and the probe, shared with a SHELL extraction, are most of the call; on small ones the ~300 queued launches of a merged call
// are.  The head-flag and gather passes are plain coalesced global passes: each reads its neighbour's key once (served by L2),
// which LDS staging would not reduce.
//   memory   per voxel: the list 16 B, its key 4 B, the face word 4 B, the counts 24 B (+ scan scratch); per exposed face: two
//            (key, value) pairs 16 B, flag / run number 4 B, start 4 B; per run the same 24 B; per quad 32 B; the sort's
//            histograms 1 KiB per 2048 items of the largest segment.
#include <algorithm>
#include <string>
#include <vector>

#include "device_scan.hpp"
#include "region_device.hpp"
#include "surface_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

// mask[i]: bit f = face f of voxel i is exposed and the voxel is inside the union of the shapes; cnt[f * (n + 1) + i] = that bit,
// cnt[f * (n + 1) + n] = 0
__global__ __launch_bounds__(256) void surface_probe_kernel(const int4 *v, const uint32_t *keys, uint32_t n, int depth, const RegionShape *shapes,
                                                            uint32_t n_shapes, uint32_t *mask, uint32_t *cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  const size_t stride = (size_t)n + 1;
  if (i == n) {
#pragma unroll
    for (int f = 0; f < 6; f++) cnt[f * stride + n] = 0u;
    return;
  }
  const int4 p = v[i];
  const uint32_t k = keys[i];
  const int N = 1 << depth;
  bool in = n_shapes == 0u;
  for (uint32_t s = 0; s < n_shapes && !in; s++) in = region_inside(shapes[s], p.x, p.y, p.z);
  uint32_t m = 0;
  if (in) {
#pragma unroll 1
    for (int f = 0; f < 6; f++) {
      const int d = (f & 1) ? 1 : -1, a = f >> 1;
      const int x = p.x + (a == 0 ? d : 0), y = p.y + (a == 1 ? d : 0), z = p.z + (a == 2 ? d : 0);
      if (x < 0 || y < 0 || z < 0 || x >= N || y >= N || z >= N || gallop_find(keys, (int)n, (int)i, k, region_key(x, y, z)) < 0) m |= 1u << f;
    }
  }
  mask[i] = m;
#pragma unroll
  for (int f = 0; f < 6; f++) cnt[f * stride + i] = (m >> f) & 1u;
}

// out[t] = excl[idx.at[t]], t = 0..6: the segment bounds one level down
__global__ void surface_bounds_kernel(const uint32_t *excl, SurfaceSegs idx, uint32_t *out) {
  if (threadIdx.x < 7u) out[threadIdx.x] = excl[idx.at[threadIdx.x]];
}

// lane i writes its exposed faces at their scanned positions; stacked = 0: (w << 20 | v << 10 | u, material), the order of the
// runs; 1: (w << 20 | u << 10 | v, u << 8 | material), the order and payload of the stacks (merge = 0)
__global__ __launch_bounds__(256) void surface_emit_kernel(const int4 *v, const uint32_t *mask, const uint32_t *excl, uint32_t n, int by_material,
                                                           int stacked, uint32_t *fk, uint32_t *fv) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = mask[i];
  if (!m) return;
  const int4 p = v[i];
  const size_t stride = (size_t)n + 1;
  const uint32_t mat = by_material ? (uint32_t)p.w : 0u;
#pragma unroll
  for (int f = 0; f < 6; f++) {
    if (!((m >> f) & 1u)) continue;
    const int a = f >> 1;
    const uint32_t w = (uint32_t)(a == 0 ? p.x : a == 1 ? p.y : p.z), u = (uint32_t)(a == 0 ? p.y : a == 1 ? p.z : p.x),
                   t = (uint32_t)(a == 0 ? p.z : a == 1 ? p.x : p.y);
    const uint32_t pos = excl[f * stride + i];
    fk[pos] = stacked ? (w << 20 | u << 10 | t) : (w << 20 | t << 10 | u);
    fv[pos] = stacked ? (u << 8 | mat) : mat;
  }
}

// flag[j] = item j starts a run (a stack): the first of its segment, not the successor of the previous key, its low field 0,
// or another value; flag[n] = 0
__global__ __launch_bounds__(256) void surface_head_flags_kernel(const uint32_t *k, const uint32_t *val, uint32_t n, SurfaceSegs segs, uint32_t *flag) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > n) return;
  if (j == n) { flag[n] = 0u; return; }
  const uint32_t key = k[j];
  bool head = j == surface_seg_start(segs, j) || (key & 1023u) == 0u;
  if (!head) head = k[j - 1u] + 1u != key || val[j - 1u] != val[j];
  flag[j] = head ? 1u : 0u;
}

// start[r] = the position of the head of run (stack) r; start[excl[n]] = n
__global__ __launch_bounds__(256) void surface_starts_kernel(const uint32_t *excl, uint32_t n, uint32_t *start) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > n) return;
  if (j == n || excl[j + 1u] != excl[j]) start[excl[j]] = j;
}

// run r -> (w << 20 | u0 << 10 | v, u1 << 8 | material)
__global__ __launch_bounds__(256) void surface_runs_kernel(const uint32_t *fk, const uint32_t *fv, const uint32_t *start, uint32_t n_runs, uint32_t *rk,
                                                           uint32_t *rv) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_runs) return;
  const uint32_t s = start[r], len = start[r + 1u] - s, key = fk[s];
  const uint32_t w = key >> 20, t = (key >> 10) & 1023u, u0 = key & 1023u;
  rk[r] = w << 20 | u0 << 10 | t;
  rv[r] = (u0 + len - 1u) << 8 | fv[s];
}

// quad q: its first run and its length (start == null: item q alone) -> tdt_quad; segs: the segments of the items
__global__ __launch_bounds__(256) void surface_quads_kernel(const uint32_t *rk, const uint32_t *rv, const uint32_t *start, uint32_t n_quads,
                                                            SurfaceSegs segs, int4 *quads) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= n_quads) return;
  const uint32_t s = start ? start[q] : q, len = start ? start[q + 1u] - s : 1u;
  const uint32_t key = rk[s], val = rv[s];
  const int f = surface_seg_of(segs, s), a = f >> 1;
  const int w = (int)(key >> 20) + (f & 1), u0 = (int)((key >> 10) & 1023u), v0 = (int)(key & 1023u);
  const int u1 = (int)(val >> 8);
  const int x = a == 0 ? w : a == 1 ? v0 : u0, y = a == 0 ? u0 : a == 1 ? w : v0, z = a == 0 ? v0 : a == 1 ? u0 : w;
  quads[2u * (size_t)q] = make_int4(f, (int)(val & 255u), x, y);
  quads[2u * (size_t)q + 1u] = make_int4(z, u1 - u0 + 1, (int)len, 0);
}

namespace {

const char *kNoMemory = "out of device memory in the surface extraction";

struct Request {
  tdt_surface s;
  std::vector<RegionShape> shapes;
};

int make_request(tdt_ctx *ctx, const tdt_surface *s, const tdt_region *regions, size_t n_regions, Request &R) {
  if (!s) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_surface pointer");
  if (s->merge != 0 && s->merge != 1) return fail(ctx, TDT_ERR_INVALID_VALUE, "merge must be 0 or 1");
  if (s->by_material != 0 && s->by_material != 1) return fail(ctx, TDT_ERR_INVALID_VALUE, "by_material must be 0 or 1");
  R.s = *s;
  return region_shapes(ctx, regions, n_regions, &R.shapes);
}

struct Pass {
  tdt_ctx *front; hipStream_t st;
  uint32_t *d_bounds;                                    // seven words the stream writes
  uint32_t *hist = nullptr, *hscr = nullptr;             // the sorts' scratch, sized for the first (largest) sort

  // segs.at[t] = excl[idx.at[t]]: ONE host synchronisation
  int read_bounds(const uint32_t *excl, const SurfaceSegs &idx, SurfaceSegs &segs) {
    hipLaunchKernelGGL(surface_bounds_kernel, dim3(1), dim3(64), 0, st, excl, idx, d_bounds);
    TDT_HIP(front, hipGetLastError());
    TDT_HIP(front, hipMemcpyAsync(segs.at, d_bounds, sizeof segs.at, hipMemcpyDeviceToHost, st));
    TDT_HIP(front, hipStreamSynchronize(st));
    return TDT_OK;
  }
  // every segment of (k, v) sorted by key in place (four radix passes leave a segment where it was); alt: a second pair
  int sort_segments(uint32_t *k, uint32_t *v, uint32_t *k_alt, uint32_t *v_alt, const SurfaceSegs &segs) {
    for (int f = 0; f < 6; f++) {
      const uint32_t lo = segs.at[f], n = segs.at[f + 1] - lo;
      uint32_t *sk = k + lo, *sv = v + lo;
      TDT_HIP(front, sort_pairs_u32(st, sk, sv, k_alt + lo, v_alt + lo, n, hist, hscr));
      if (sk != k + lo) return fail(front, TDT_ERR_HIP, "the radix sort left a segment in its second buffer");
    }
    return TDT_OK;
  }
  // heads of (k, v) over segs flagged and numbered (flag: n + 1 words, scanned in place), their positions in start (n + 1 words)
  int number_heads(const uint32_t *k, const uint32_t *v, uint32_t n, const SurfaceSegs &segs, uint32_t *flag, uint32_t *scr, uint32_t *start) {
    hipLaunchKernelGGL(surface_head_flags_kernel, dim3(blocks_of((size_t)n + 1)), dim3(256), 0, st, k, v, n, segs, flag);
    TDT_HIP(front, exclusive_scan_u32(st, flag, flag, n + 1u, scr));
    hipLaunchKernelGGL(surface_starts_kernel, dim3(blocks_of((size_t)n + 1)), dim3(256), 0, st, (const uint32_t *)flag, n, start);
    return TDT_OK;
  }
};

// the quads of one single-device context's tree, in device memory of ctx (allocated in S; null when *n == 0)
int surface_quads(tdt_ctx *front, tdt_ctx *ctx, const Request &R, DeviceScratch &S, const int4 **out, uint32_t *n_out) {
  *out = nullptr; *n_out = 0;
  hipStream_t st = ctx->stream;
  // ---- probe, emit, sort: the faces, numbered direction by direction ----
  SurfaceFaces L;
  if (int rc = surface_face_list(front, ctx, R.shapes, R.s.by_material, R.s.merge ? 0 : 1, S, L)) return rc;
  const uint32_t nf = L.nf;
  if (nf == 0) return TDT_OK;
  Pass P{front, st, L.d_bounds, L.hist, L.hscr};
  const SurfaceSegs &faces = L.segs;
  uint32_t *fk = L.fk, *fv = L.fv, *fk_alt = L.fk_alt, *fv_alt = L.fv_alt;
  const uint32_t *qk = fk, *qv = fv, *q_start = nullptr;                   // what the quads are written from
  SurfaceSegs q_segs = faces;
  uint32_t nq = nf;
  if (R.s.merge) {
    // ---- runs ----
    uint32_t *flag = S.get<uint32_t>((size_t)nf + 1), *fscr = S.get<uint32_t>(scan_scratch_words((size_t)nf + 1)), *start = S.get<uint32_t>((size_t)nf + 1);
    if (!flag || !fscr || !start) return fail(front, TDT_ERR_HIP, kNoMemory);
    if (int rc = P.number_heads(fk, fv, nf, faces, flag, fscr, start)) return rc;
    SurfaceSegs runs;
    if (int rc = P.read_bounds(flag, faces, runs)) return rc;              // runs do not cross segments: a segment's first item is a head
    const uint32_t nr = runs.at[6];                                        // 1 <= nr <= nf: the sorts' scratch is large enough
    // ---- stacks: the faces' second pair is free now, and long enough ----
    uint32_t *rk = fk_alt, *rv = fv_alt;
    uint32_t *rk_alt = S.get<uint32_t>(nr), *rv_alt = S.get<uint32_t>(nr);
    uint32_t *rflag = S.get<uint32_t>((size_t)nr + 1), *rscr = S.get<uint32_t>(scan_scratch_words((size_t)nr + 1)), *rstart = S.get<uint32_t>((size_t)nr + 1);
    if (!rk_alt || !rv_alt || !rflag || !rscr || !rstart) return fail(front, TDT_ERR_HIP, kNoMemory);
    hipLaunchKernelGGL(surface_runs_kernel, dim3(blocks_of(nr)), dim3(256), 0, st, (const uint32_t *)fk, (const uint32_t *)fv, (const uint32_t *)start, nr,
                       rk, rv);
    if (int rc = P.sort_segments(rk, rv, rk_alt, rv_alt, runs)) return rc;
    if (int rc = P.number_heads(rk, rv, nr, runs, rflag, rscr, rstart)) return rc;
    SurfaceSegs quads;
    if (int rc = P.read_bounds(rflag, runs, quads)) return rc;
    qk = rk; qv = rv; q_start = rstart; q_segs = runs; nq = quads.at[6];
  }
  // ---- quads ----
  int4 *d_quads = S.get<int4>(2 * (size_t)nq);
  if (!d_quads) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(surface_quads_kernel, dim3(blocks_of(nq)), dim3(256), 0, st, qk, qv, q_start, nq, q_segs, d_quads);
  TDT_HIP(front, hipGetLastError());
  *out = d_quads; *n_out = nq;
  return TDT_OK;
}

}  // namespace

int surface_face_list(tdt_ctx *front, tdt_ctx *ctx, const std::vector<RegionShape> &shapes, int by_material, int stacked, DeviceScratch &S,
                      SurfaceFaces &L) {
  L = SurfaceFaces{};
  hipStream_t st = ctx->stream;
  if (int rc = tree_voxels_capped(front, ctx, S, &L.v, &L.nv, &L.depth)) return rc;
  const uint32_t nv = L.nv;
  if (nv == 0) return TDT_OK;
  int4 *v = L.v;
  // ---- probe: the faces, numbered direction by direction ----
  const size_t stride = (size_t)nv + 1, n_cnt = 6 * stride;                // < 2^32: nv <= 2^26
  uint32_t *keys = S.get<uint32_t>(nv), *mask = S.get<uint32_t>(nv), *cnt = S.get<uint32_t>(n_cnt), *scr = S.get<uint32_t>(scan_scratch_words(n_cnt));
  uint32_t *d_bounds = S.get<uint32_t>(7);
  RegionShape *d_shapes = nullptr;
  if (!keys || !mask || !cnt || !scr || !d_bounds) return fail(front, TDT_ERR_HIP, kNoMemory);
  L.keys = keys; L.d_bounds = d_bounds;
  const uint32_t n_shapes = (uint32_t)shapes.size();
  if (int rc = upload_shapes(front, st, S, shapes.data(), n_shapes, kNoMemory, &d_shapes)) return rc;
  voxlist_keys(st, v, nv, keys);
  hipLaunchKernelGGL(surface_probe_kernel, dim3(blocks_of(stride)), dim3(256), 0, st, (const int4 *)v, (const uint32_t *)keys, nv, L.depth,
                     (const RegionShape *)d_shapes, n_shapes, mask, cnt);
  TDT_HIP(front, exclusive_scan_u32(st, cnt, cnt, (uint32_t)n_cnt, scr));
  Pass P{front, st, d_bounds};
  SurfaceSegs idx, faces;
  for (int f = 0; f < 6; f++) idx.at[f] = (uint32_t)(f * stride);
  idx.at[6] = (uint32_t)(n_cnt - 1);                                       // the last direction's closing 0: the total
  if (int rc = P.read_bounds(cnt, idx, faces)) return rc;
  const uint32_t nf = faces.at[6];
  for (int f = 0; f < 6; f++)
    if (faces.at[f + 1] - faces.at[f] > kVoxelListCap)
      return fail(front, TDT_ERR_INVALID_VALUE, "direction " + std::to_string(f) + " has " + std::to_string(faces.at[f + 1] - faces.at[f]) +
                                                    " exposed faces (more than 2^26)");
  L.segs = faces; L.nf = nf;
  if (nf == 0) return TDT_OK;
  // ---- emit, sort ----
  uint32_t largest = 0;
  for (int f = 0; f < 6; f++) largest = std::max(largest, faces.at[f + 1] - faces.at[f]);
  uint32_t *fk = S.get<uint32_t>(nf), *fv = S.get<uint32_t>(nf), *fk_alt = S.get<uint32_t>(nf), *fv_alt = S.get<uint32_t>(nf);
  P.hist = S.get<uint32_t>(sort_hist_words(largest)); P.hscr = S.get<uint32_t>(sort_scratch_words(largest));
  if (!fk || !fv || !fk_alt || !fv_alt || !P.hist || !P.hscr) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(surface_emit_kernel, dim3(blocks_of(nv)), dim3(256), 0, st, (const int4 *)v, (const uint32_t *)mask, (const uint32_t *)cnt, nv,
                     by_material, stacked, fk, fv);
  if (int rc = P.sort_segments(fk, fv, fk_alt, fv_alt, faces)) return rc;
  TDT_HIP(front, hipGetLastError());
  L.fk = fk; L.fv = fv; L.fk_alt = fk_alt; L.fv_alt = fv_alt; L.hist = P.hist; L.hscr = P.hscr;
  return TDT_OK;
}

void surface_unit_quads(hipStream_t st, const uint32_t *fk, const uint32_t *fv, uint32_t n, const SurfaceSegs &segs, int4 *quads) {
  hipLaunchKernelGGL(surface_quads_kernel, dim3(blocks_of(n)), dim3(256), 0, st, fk, fv, (const uint32_t *)nullptr, n, segs, quads);
}

}  // namespace tdt

extern "C" {

int tdt_octree_extract_surface(tdt_ctx *ctx, const tdt_surface *opt, const tdt_region *regions, size_t n_regions, tdt_quad *quads,
                               size_t capacity, size_t *n_quads) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_quads) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_quads pointer");
  *n_quads = 0;
  Request R;
  if (int rc = make_request(ctx, opt, regions, n_regions, R)) return rc;
  tdt_ctx *m = first_member(ctx);
  TDT_HIP(ctx, hipSetDevice(m->device));
  DeviceScratch S;
  Drain drain{m->stream};                                // before S is freed
  const int4 *d_quads = nullptr;
  uint32_t n = 0;
  if (int rc = surface_quads(ctx, m, R, S, &d_quads, &n)) return rc;
  return list_to_host(ctx, m->stream, d_quads, n, sizeof(tdt_quad), "quads", quads, capacity, n_quads);
}

}  // extern "C"
