// Region edits — set / fill / paint / clear a box, a sphere, a union of them or a voxel list, on any tree the library renders
// (include/tdt_rt.h tdt_octree_edit_region / tdt_octree_edit_voxels / tdt_octree_extract_region).  An edit is compaction
// (tdt_compact.hip) with a set operation applied to the voxel list before the rebuild:
//
//   V        the walk of the bound tree, expanded to its Morton-sorted voxel list (tree_voxels); keys  one lane per voxel
//   B        shapes (SET / FILL): one lane per candidate of each shape's grid-clipped bounding box runs the shape test, a wave64
//            ballot + popcount compacts the hits into (Morton key, material) pairs behind one atomic per wave.  Voxel list:
//            one lane per voxel -> key (off-grid: the all-ones "dropped" key); the list comes from the host, or from a
//            VoxelSource that produced it in device memory (tdt_mesh.hip: a rasterised mesh).  Then the builder's stable radix sort and a
//            last-of-each-run unique.  Queued before the walk, so the walk's one host synchronisation also reads |B raw|.
//            PAINT / CLEAR with shapes build no B: the merge tests each voxel of V against the shapes instead (cost |V|), or
//            reads a per-voxel membership a VoxelSelect computed on V (connected components, tdt_connect.hip).
//   merge    rank merge: a V lane binary-searches B (lower bound j, slot i + j), a B lane binary-searches V (upper bound i,
//            slot i + j): V before B on equal keys, so the slots are a permutation of the merged order.  The op table sets
//            each slot's keep flag and voxel; exclusive_scan_u32 over the flags and one compaction give the result, sorted.
//            One host synchronisation reads its length.
//   rebuild  build_cells_from_device + install_cells: compaction's fit check and in-place install.
#include <cstring>
#include <string>
#include <vector>

#include "device_scan.hpp"
#include "region_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr int kOpIntersect = 4;                    // extract_region: keep V inside the shapes

// one lane per candidate voxel of every shape's clipped box; hits -> (key, m) behind one atomic per wave
__global__ __launch_bounds__(256) void region_brush_kernel(const RegionShape *shapes, uint32_t n_shapes, uint32_t n_lanes, uint32_t m,
                                                          uint32_t *keys, uint32_t *vals, uint32_t *count) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  bool hit = false;
  uint32_t key = 0;
  if (g < n_lanes) {
    uint32_t lo = 0, hi = n_shapes;                          // the last shape whose first lane is <= g
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (shapes[mid].lane0 <= g) lo = mid; else hi = mid; }
    const RegionShape &s = shapes[lo];
    const uint32_t l = g - s.lane0, yz = s.ext[1] * s.ext[2];
    const int x = s.lo[0] + (int)(l / yz), y = s.lo[1] + (int)((l % yz) / s.ext[2]), z = s.lo[2] + (int)(l % s.ext[2]);
    hit = region_inside(s, x, y, z);
    key = region_key(x, y, z);
  }
  const unsigned long long ball = __ballot(hit);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0 && ball) base = atomicAdd(count, (uint32_t)__popcll(ball));
  base = (uint32_t)__shfl((int)base, 0, 64);
  if (hit) {
    const uint32_t pos = base + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
    keys[pos] = key; vals[pos] = m;
  }
}

// voxel-list form: {x, y, z, m} -> (key, m); off-grid -> dropped
__global__ __launch_bounds__(256) void region_list_keys_kernel(const int4 *vox, uint32_t n, int depth, bool clear, uint32_t *keys, uint32_t *vals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 v = vox[i];
  const int N = 1 << depth;
  const bool ok = v.x >= 0 && v.y >= 0 && v.z >= 0 && v.x < N && v.y < N && v.z < N;
  keys[i] = ok ? region_key(v.x, v.y, v.z) : kDroppedKey;
  vals[i] = clear ? 0u : (uint32_t)v.w;
}

struct MergeArgs {
  const int4 *v; const uint32_t *kv; uint32_t nv;
  const uint32_t *kb, *mb, *nb;                 // B (kb null: test V against the shapes)
  const RegionShape *shapes; uint32_t n_shapes; uint32_t m;
  const uint32_t *label, *selected;             // a membership (VoxelSelect) in place of the shapes: selected[label[i]] != 0
  int op;
  int4 *slot; uint32_t *keep;                   // nv + |B| slots (keep zeroed beforehand)
};

// a V lane: slot i + (B keys below), keep / voxel by the op table
__global__ __launch_bounds__(256) void region_merge_v_kernel(const MergeArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.nv) return;
  const int4 p = A.v[i];
  bool in = false;
  uint32_t pos = i, bm = A.m;
  if (A.kb) {
    const uint32_t k = A.kv[i], nb = *A.nb, lo = lower_bound_u32(A.kb, nb, k);
    in = lo < nb && A.kb[lo] == k;
    if (in) bm = A.mb[lo];
    pos = i + lo;
  } else if (A.selected) {
    in = A.selected[A.label[i]] != 0u;
  } else {
    for (uint32_t s = 0; s < A.n_shapes && !in; s++) in = region_inside(A.shapes[s], p.x, p.y, p.z);
  }
  bool keep;
  int m = p.w;
  switch (A.op) {
    case TDT_REGION_SET: case TDT_REGION_CLEAR: keep = !in; break;
    case TDT_REGION_PAINT: keep = true; if (in) m = (int)bm; break;
    case kOpIntersect: keep = in; break;
    default: keep = true; break;                  // FILL: V stays
  }
  A.keep[pos] = keep ? 1u : 0u;
  if (keep) A.slot[pos] = make_int4(p.x, p.y, p.z, m);
}

// a B lane (SET / FILL only): slot j + (V keys at or below)
__global__ __launch_bounds__(256) void region_merge_b_kernel(const MergeArgs A) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= *A.nb) return;
  const uint32_t k = A.kb[j], lo = upper_bound_u32(A.kv, A.nv, k);
  const bool in_v = lo > 0 && A.kv[lo - 1u] == k;
  const bool keep = A.op == TDT_REGION_SET || !in_v;
  const uint32_t pos = lo + j;
  A.keep[pos] = keep ? 1u : 0u;
  if (keep) A.slot[pos] = region_voxel(k, (int)A.mb[j]);
}

namespace {

const char *kNoMemory = "out of device memory in the region edit";

// what one call asks for, validated on the host before anything is queued
struct Request {
  int op = TDT_REGION_SET;
  const tdt_region *regions = nullptr; size_t n_regions = 0;
  int32_t material = 0;                         // shapes: 0..253
  const int32_t *vox = nullptr; size_t n_vox = 0; bool list = false;
  VoxelSelect *select = nullptr;                // PAINT / CLEAR / intersect of the voxels it selects (no shapes)
  VoxelSource *source = nullptr;                // list form: the list is produced in device memory (vox / n_vox unused)
};

int check_request(tdt_ctx *ctx, const Request &R) {
  if (R.op < TDT_REGION_SET || R.op > kOpIntersect) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  if (R.list && R.source) return TDT_OK;           // a device-resident list: its producer has checked its input
  if (R.list) {
    if (R.n_vox && !R.vox) return fail(ctx, TDT_ERR_INVALID_VALUE, "null voxel list");
    if (R.n_vox >= (1ull << 31)) return fail(ctx, TDT_ERR_INVALID_VALUE, "more than 2^31 voxels");
    if (R.op != TDT_REGION_CLEAR)
      for (size_t i = 0; i < R.n_vox; i++)
        if (R.vox[4 * i + 3] < 1 || R.vox[4 * i + 3] > 254)
          return fail(ctx, TDT_ERR_INVALID_VALUE, "voxel " + std::to_string(i) + ": m must be 1..254");
    return TDT_OK;
  }
  if (R.n_regions && !R.regions) return fail(ctx, TDT_ERR_INVALID_VALUE, "null region list");   // (ahead of the material, as ever)
  if (R.material < 0 || R.material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be 0..253");
  return region_shapes(ctx, R.regions, R.n_regions, nullptr);    // clip_shapes makes the shapes, once the depth is known
}

// the shapes with their bounding boxes clipped to a grid of side N; *lanes = the candidates of all of them
void clip_shapes(const Request &R, int depth, std::vector<RegionShape> &out, unsigned long long *lanes) {
  const long long N = 1ll << depth;
  *lanes = 0;
  out.clear();
  for (size_t s = 0; s < R.n_regions; s++) {
    const tdt_region &g = R.regions[s];
    RegionShape r;
    std::memset(&r, 0, sizeof r);
    r.shape = g.shape;
    for (int a = 0; a < 3; a++) { r.a[a] = g.a[a]; r.b[a] = g.b[a]; }
    unsigned long long n = 1;
    for (int a = 0; a < 3; a++) {
      long long lo = g.shape == TDT_SHAPE_BOX ? g.a[a] : (long long)g.a[a] - g.b[0];
      long long hi = g.shape == TDT_SHAPE_BOX ? g.b[a] : (long long)g.a[a] + g.b[0];
      lo = lo < 0 ? 0 : lo; hi = hi > N - 1 ? N - 1 : hi;
      const unsigned long long e = hi >= lo ? (unsigned long long)(hi - lo + 1) : 0ull;
      r.lo[a] = (int32_t)lo; r.ext[a] = (uint32_t)e; n *= e;
    }
    if (n == 0) continue;                              // nothing of it in the grid
    r.lane0 = (uint32_t)(*lanes < kVoxelListCap ? *lanes : 0);
    *lanes += n;
    out.push_back(r);
  }
}

// one single-device context: the edit (or, op == kOpIntersect, V ∩ B into host memory)
int region_one(tdt_ctx *front, tdt_ctx *ctx, const Request &R, uint32_t *n_cells, int32_t *host_out, size_t capacity, size_t *n_out) {
  int depth = 0;
  if (int rc = walk_inputs(front, ctx, &depth)) return rc;
  std::vector<RegionShape> shapes;
  unsigned long long lanes = 0;
  if (!R.list) {
    clip_shapes(R, depth, shapes, &lanes);
    if ((R.op == TDT_REGION_SET || R.op == TDT_REGION_FILL) && lanes > kVoxelListCap)
      return fail(front, TDT_ERR_INVALID_VALUE, "the shapes enumerate " + std::to_string(lanes) + " candidate voxels (more than 2^26)");
  }
  hipStream_t st = ctx->stream;
  TDT_HIP(front, hipSetDevice(ctx->device));
  uint32_t b_raw = 0, n_res = 0;                          // host words the stream writes: the guard below outlives them
  Drain drain{st};
  DeviceScratch S;
  const int4 *src_vox = nullptr;                          // the device-resident list
  uint32_t src_n = 0;
  if (R.source)
    if (int rc = R.source->run(front, ctx, depth, S, &src_vox, &src_n)) return rc;
  // ---- B, queued before the walk ----
  const bool build_b = R.list || ((R.op == TDT_REGION_SET || R.op == TDT_REGION_FILL) && lanes > 0);
  const uint32_t b_cap = R.source ? src_n : R.list ? (uint32_t)R.n_vox : (uint32_t)lanes;
  uint32_t *bk = nullptr, *bv = nullptr, *bk_alt = nullptr, *bv_alt = nullptr, *b_count = nullptr;
  RegionShape *d_shapes = nullptr;
  b_raw = b_cap;
  if (int rc = upload_shapes(front, st, S, shapes.data(), shapes.size(), kNoMemory, &d_shapes)) return rc;
  if (build_b && b_cap) {
    bk = S.get<uint32_t>(b_cap); bv = S.get<uint32_t>(b_cap); bk_alt = S.get<uint32_t>(b_cap); bv_alt = S.get<uint32_t>(b_cap);
    b_count = S.get<uint32_t>(2);
    if (!bk || !bv || !bk_alt || !bv_alt || !b_count) return fail(front, TDT_ERR_HIP, kNoMemory);
    TDT_HIP(front, hipMemsetAsync(b_count, 0, 2 * sizeof(uint32_t), st));
    if (R.source) {
      hipLaunchKernelGGL(region_list_keys_kernel, dim3(blocks_of(b_cap)), dim3(256), 0, st, src_vox, b_cap, depth, R.op == TDT_REGION_CLEAR, bk, bv);
    } else if (R.list) {
      int4 *d_vox = S.get<int4>(b_cap);
      if (!d_vox) return fail(front, TDT_ERR_HIP, kNoMemory);
      TDT_HIP(front, hipMemcpyAsync(d_vox, R.vox, (size_t)b_cap * sizeof(int4), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(region_list_keys_kernel, dim3(blocks_of(b_cap)), dim3(256), 0, st, (const int4 *)d_vox, b_cap, depth,
                         R.op == TDT_REGION_CLEAR, bk, bv);
    } else {
      hipLaunchKernelGGL(region_brush_kernel, dim3(blocks_of(b_cap)), dim3(256), 0, st, (const RegionShape *)d_shapes, (uint32_t)shapes.size(),
                         b_cap, (uint32_t)R.material + 1u, bk, bv, b_count);
      TDT_HIP(front, hipMemcpyAsync(&b_raw, b_count, sizeof b_raw, hipMemcpyDeviceToHost, st));   // read at the walk's synchronisation
    }
    TDT_HIP(front, hipGetLastError());
  }
  // ---- V ----
  int4 *v = nullptr;
  uint32_t nv = 0;
  if (int rc = tree_voxels(front, ctx, R.op == kOpIntersect ? 0x7FFFFFFFu : 254u, S, &v, &nv, &depth)) return rc;
  const uint32_t *label = nullptr, *selected = nullptr;
  if (R.select && nv)
    if (int rc = R.select->run(front, ctx, v, nv, depth, S, &label, &selected)) return rc;
  // ---- sort and unique B ----
  uint32_t *kb = nullptr, *mb = nullptr, *nb = nullptr;
  if (build_b && b_cap && b_raw) {
    uint32_t *hist = S.get<uint32_t>(sort_hist_words(b_raw)), *hscr = S.get<uint32_t>(sort_scratch_words(b_raw));
    uint32_t *flag = S.get<uint32_t>((size_t)b_raw + 1), *fscr = S.get<uint32_t>(scan_scratch_words((size_t)b_raw + 1));
    if (!hist || !hscr || !flag || !fscr) return fail(front, TDT_ERR_HIP, kNoMemory);
    uint32_t *k = bk, *vv = bv;
    TDT_HIP(front, sort_pairs_u32(st, k, vv, bk_alt, bv_alt, b_raw, hist, hscr));
    kb = k == bk ? bk_alt : bk; mb = vv == bv ? bv_alt : bv; nb = b_count + 1;   // the pair the sort left free
    voxlist_last_flags(st, k, b_raw, flag);
    TDT_HIP(front, exclusive_scan_u32(st, flag, flag, b_raw + 1u, fscr));
    voxlist_unique(st, k, vv, b_raw, flag, kb, mb, nb);
  }
  // ---- merge ----
  const unsigned long long n_slots = (unsigned long long)nv + (kb ? b_raw : 0u);
  if (n_slots >= (1ull << 31)) return fail(front, TDT_ERR_INVALID_VALUE, "the merged voxel list is too large");
  int4 *res = nullptr;
  if (n_slots) {
    uint32_t *kv = S.get<uint32_t>(nv), *keep = S.get<uint32_t>(n_slots + 1), *kscr = S.get<uint32_t>(scan_scratch_words(n_slots + 1));
    int4 *slot = S.get<int4>(n_slots);
    res = S.get<int4>(n_slots);
    uint32_t *d_res = S.get<uint32_t>(1);
    if (!kv || !keep || !kscr || !slot || !res || !d_res) return fail(front, TDT_ERR_HIP, kNoMemory);
    TDT_HIP(front, hipMemsetAsync(keep, 0, (n_slots + 1) * sizeof(uint32_t), st));
    MergeArgs A;
    std::memset(&A, 0, sizeof A);
    A.v = v; A.kv = kv; A.nv = nv; A.kb = kb; A.mb = mb; A.nb = nb;
    A.shapes = d_shapes; A.n_shapes = (uint32_t)shapes.size(); A.m = (uint32_t)R.material + 1u; A.op = R.op;
    A.label = label; A.selected = selected;
    A.slot = slot; A.keep = keep;
    if (nv) {
      if (kb) voxlist_keys(st, v, nv, kv);
      hipLaunchKernelGGL(region_merge_v_kernel, dim3(blocks_of(nv)), dim3(256), 0, st, A);
    }
    if (kb && (R.op == TDT_REGION_SET || R.op == TDT_REGION_FILL))
      hipLaunchKernelGGL(region_merge_b_kernel, dim3(blocks_of(b_raw)), dim3(256), 0, st, A);
    if (int rc = scan_gather_count(front, st, slot, nullptr, keep, (uint32_t)n_slots, kscr, res, nullptr, &n_res)) return rc;   // the merged count
  }
  if (R.op == kOpIntersect) return list_to_host(front, st, res, n_res, sizeof(int4), "voxels", host_out, capacity, n_out);
  // ---- rebuild and install ----
  return rebuild_install(front, ctx, res, n_res, depth, true, n_cells, [&] { S.release(); });
}

// an edit of every replica, a misfit reporting the size to grow to
int region_edit(tdt_ctx *ctx, const Request &R, uint32_t *n_cells) {
  if (int rc = check_request(ctx, R)) return rc;
  return edit_replicas(ctx, true, n_cells, [&](tdt_ctx *m, uint32_t *nc) { return region_one(ctx, m, R, nc, nullptr, 0, nullptr); });
}

}  // namespace

int region_edit_selected(tdt_ctx *ctx, int op, int32_t material, VoxelSelect &sel, uint32_t *n_cells) {
  Request R;
  R.op = op; R.material = material; R.select = &sel;
  return region_edit(ctx, R, n_cells);
}

int region_edit_source(tdt_ctx *ctx, int op, VoxelSource &src, uint32_t *n_cells) {
  Request R;
  R.op = op; R.list = true; R.source = &src;
  return region_edit(ctx, R, n_cells);
}

int region_intersect_source(tdt_ctx *ctx, VoxelSource &src, int32_t *host_out, size_t capacity, size_t *n_out) {
  Request R;
  R.op = kOpIntersect; R.list = true; R.source = &src;
  return region_one(ctx, first_member(ctx), R, nullptr, host_out, capacity, n_out);
}

int region_extract_selected(tdt_ctx *ctx, VoxelSelect &sel, int32_t *host_out, size_t capacity, size_t *n_out) {
  Request R;
  R.op = kOpIntersect; R.select = &sel;
  return region_one(ctx, first_member(ctx), R, nullptr, host_out, capacity, n_out);
}

}  // namespace tdt

extern "C" {

int tdt_octree_edit_region(tdt_ctx *ctx, int op, const tdt_region *regions, size_t n_regions, int32_t material, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (op < TDT_REGION_SET || op > TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  Request R;
  R.op = op; R.regions = regions; R.n_regions = n_regions; R.material = material;
  return region_edit(ctx, R, n_cells);
}

int tdt_octree_edit_voxels(tdt_ctx *ctx, int op, const int32_t *voxels_xyzm, size_t n, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (op < TDT_REGION_SET || op > TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  Request R;
  R.op = op; R.vox = voxels_xyzm; R.n_vox = n; R.list = true;
  return region_edit(ctx, R, n_cells);
}

int tdt_octree_extract_region(tdt_ctx *ctx, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  Request R;
  R.op = kOpIntersect; R.regions = regions; R.n_regions = n_regions;
  if (int rc = check_request(ctx, R)) return rc;
  return region_one(ctx, first_member(ctx), R, nullptr, voxels_xyzm, capacity, n_voxels);
}

}  // extern "C"
