// Voxel morphology — grow, shrink, open, close, hollow (include/tdt_rt.h tdt_octree_morph / tdt_octree_extract_morph).  All r
// steps run on the Morton-sorted voxel list (tree_voxels) and its keys; the tree is rebuilt once at the end.
//
//   probe    one lane per voxel of the current list: the 6 / 26 neighbour keys looked up with gallop_find (Morton neighbours are
//            mostly near the lane's own index).  One word per voxel: bit t(d) set = the in-grid neighbour at offset d is absent;
//            bit 13 (the centre's number, otherwise unused) = some neighbour is outside the grid.  The same launch writes the
//            count the step scans: erode 1 / 0 (keep), dilate popc(absent).
//   erode    exclusive_scan_u32 over the keep flags, one gather of voxels and keys.  ONE host synchronisation (the length).
//   dilate   exclusive_scan_u32 over the counts (synchronisation: the candidate total sizes the next launches); emit: lane i
//            writes its candidates at excl[i].. in ascending t — (candidate key, t as seen from the candidate << 8 | the emitter's
//            material + 1), no atomics; sort_pairs_u32 by key; of each run of equal keys (at most 26 long) the head lane keeps
//            the lowest value = the lowest t = the inherit rule; a scan over the heads compacts them (synchronisation: their
//            number); rank merge into the list: a list lane takes slot i + lower_bound(new, key), a new lane slot
//            j + upper_bound(list, key) (disjoint sets).  Only voxels with an absent neighbour emit.  TWO synchronisations.
//   combine  SHELL / OPEN (subsets of V, original materials): one lane per voxel of V binary-searches the stepped list, keep =
//            not in it / in it (or outside the mask).  A mask on the other ops: rank merge of the result R and V, R before V on equal keys, keep = R inside M / V outside M.
//            Scan, gather; one synchronisation.  Otherwise the list is the result as it stands.
//   rebuild  build_cells_from_device + install_cells on every replica, as region edits do.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_scan.hpp"
#include "region_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr uint32_t kMorphOutside = 1u << 13;       // probe word: a neighbour outside the grid

// mask[i]: absent in-grid neighbours by t, kMorphOutside; cnt[i]: dilate popc(absent), erode keep (border: outside is solid);
// cnt[n] = 0 (an exclusive scan over n + 1 leaves the total in [n])
template <int CONN>
__global__ __launch_bounds__(256) void morph_probe_kernel(const int4 *v, const uint32_t *keys, uint32_t n, int depth, int erode, int border,
                                                          uint32_t *mask, uint32_t *cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  if (i == n) { cnt[n] = 0u; return; }
  const int4 p = v[i];
  const uint32_t k = keys[i];
  const int N = 1 << depth;
  uint32_t m = 0;
  constexpr int kCount = CONN == 6 ? 6 : 27;
#pragma unroll 1
  for (int h = 0; h < kCount; h++) {
    const int t = CONN == 6 ? (h == 0 ? 4 : h == 1 ? 10 : h == 2 ? 12 : h == 3 ? 14 : h == 4 ? 16 : 22) : h;   // the faces, ascending
    if (t == 13) continue;
    const int x = p.x + t / 9 - 1, y = p.y + (t / 3) % 3 - 1, z = p.z + t % 3 - 1;
    if (x < 0 || y < 0 || z < 0 || x >= N || y >= N || z >= N) { m |= kMorphOutside; continue; }
    if (gallop_find(keys, (int)n, (int)i, k, region_key(x, y, z)) < 0) m |= 1u << t;
  }
  mask[i] = m;
  const uint32_t absent = m & ~kMorphOutside;
  cnt[i] = erode ? ((absent == 0u && (border || !(m & kMorphOutside))) ? 1u : 0u) : (uint32_t)__popc(absent);
}

// lane i writes its candidates at excl[i].., ascending t: (key of p + d, (26 - t(d)) << 8 | material + 1)
__global__ __launch_bounds__(256) void morph_emit_kernel(const int4 *v, const uint32_t *mask, const uint32_t *excl, uint32_t n, uint32_t *ck,
                                                         uint32_t *cv) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t m = mask[i] & ~kMorphOutside;
  if (!m) return;
  const int4 p = v[i];
  uint32_t pos = excl[i];
  while (m) {
    const int t = __ffs((int)m) - 1;
    m &= m - 1u;
    ck[pos] = region_key(p.x + t / 9 - 1, p.y + (t / 3) % 3 - 1, p.z + t % 3 - 1);
    cv[pos] = ((uint32_t)(26 - t) << 8) | (uint32_t)p.w;
    pos++;
  }
}

// flag[i] = i starts a run of equal sorted keys; flag[n] = 0
__global__ __launch_bounds__(256) void morph_head_flags_kernel(const uint32_t *k, uint32_t n, uint32_t *flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  flag[i] = (i < n && (i == 0u || k[i - 1u] != k[i])) ? 1u : 0u;
}

// a run's head lane: the run's lowest value (= lowest t) -> (key, material + 1); fixed > 0: that value instead
__global__ __launch_bounds__(256) void morph_unique_kernel(const uint32_t *k, const uint32_t *val, uint32_t n, const uint32_t *excl,
                                                           uint32_t fixed, uint32_t *uk, uint32_t *uv) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || excl[i + 1u] == excl[i]) return;
  const uint32_t key = k[i];
  uint32_t best = val[i];
  for (uint32_t j = i + 1u; j < n && k[j] == key; j++) best = min(best, val[j]);
  uk[excl[i]] = key;
  uv[excl[i]] = fixed ? fixed : (best & 0xFFu);
}

// rank merge of the list (nv) and the new voxels (nu), disjoint: both kernels write voxels and keys of the merged list
__global__ __launch_bounds__(256) void morph_merge_list_kernel(const int4 *v, const uint32_t *kv, uint32_t nv, const uint32_t *uk, uint32_t nu,
                                                               int4 *ov, uint32_t *ok) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nv) return;
  const uint32_t k = kv[i], lo = lower_bound_u32(uk, nu, k);
  ov[i + lo] = v[i]; ok[i + lo] = k;
}
__global__ __launch_bounds__(256) void morph_merge_new_kernel(const uint32_t *kv, uint32_t nv, const uint32_t *uk, const uint32_t *uv, uint32_t nu,
                                                              int4 *ov, uint32_t *ok) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= nu) return;
  const uint32_t k = uk[j], lo = upper_bound_u32(kv, nv, k);
  ov[j + lo] = region_voxel(k, (int)uv[j]);
  ok[j + lo] = k;
}

__device__ __forceinline__ bool morph_in_mask(const RegionShape *shapes, uint32_t n_shapes, const int4 &p) {
  bool in = n_shapes == 0u;
  for (uint32_t s = 0; s < n_shapes && !in; s++) in = region_inside(shapes[s], p.x, p.y, p.z);
  return in;
}

// SHELL (want 0) / OPEN (want 1): a voxel of V stays when its membership of the stepped list is `want`, or it is outside the
// mask; keep[nv] = 0
__global__ __launch_bounds__(256) void morph_select_kernel(const int4 *v, const uint32_t *kv, uint32_t nv, const uint32_t *ke, uint32_t ne,
                                                           int want, const RegionShape *shapes, uint32_t n_shapes, uint32_t *keep) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > nv) return;
  if (i == nv) { keep[nv] = 0u; return; }
  const uint32_t k = kv[i], lo = lower_bound_u32(ke, ne, k);
  const bool found = lo < ne && ke[lo] == k;
  keep[i] = (found == (want != 0) || !morph_in_mask(shapes, n_shapes, v[i])) ? 1u : 0u;
}

// the mask: (R inside M) + (V outside M) over nr + nv slots, R before V on equal keys; keep[nr + nv] = 0 (written by the R side)
__global__ __launch_bounds__(256) void morph_mask_result_kernel(const int4 *r, const uint32_t *kr, uint32_t nr, const uint32_t *kv, uint32_t nv,
                                                                const RegionShape *shapes, uint32_t n_shapes, int4 *slot, uint32_t *keep) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > nr) return;
  if (i == nr) { keep[nr + nv] = 0u; return; }
  const uint32_t lo = lower_bound_u32(kv, nv, kr[i]);
  const int4 p = r[i];
  const bool in = morph_in_mask(shapes, n_shapes, p);
  keep[i + lo] = in ? 1u : 0u;
  if (in) slot[i + lo] = p;
}
__global__ __launch_bounds__(256) void morph_mask_tree_kernel(const int4 *v, const uint32_t *kv, uint32_t nv, const uint32_t *kr, uint32_t nr,
                                                              const RegionShape *shapes, uint32_t n_shapes, int4 *slot, uint32_t *keep) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= nv) return;
  const uint32_t lo = upper_bound_u32(kr, nr, kv[j]);
  const int4 p = v[j];
  const bool in = morph_in_mask(shapes, n_shapes, p);
  keep[j + lo] = in ? 0u : 1u;
  if (!in) slot[j + lo] = p;
}

namespace {

const char *kNoMemory = "out of device memory in the voxel morphology";

// a voxel list with its keys; `mem` owns it and the temporaries of the step that made it (kernels of the NEXT step still read
// them, so a list is freed only after the step that replaced it has synchronised)
struct List {
  DeviceScratch mem;
  int4 *v = nullptr; uint32_t *k = nullptr; uint32_t n = 0;
};

struct Step {
  tdt_ctx *front, *ctx; hipStream_t st; int depth, connectivity;
  uint32_t *host_word;                                   // a host word the stream writes (outlives the stream's work)

  int read_word(const uint32_t *dev) {
    TDT_HIP(front, hipGetLastError());
    return tdt::read_word(front, st, dev, host_word);
  }
  void probe(const List &in, bool erode, int border, uint32_t *mask, uint32_t *cnt) {
    const dim3 g(blocks_of((size_t)in.n + 1)), b(256);
    if (connectivity == 6)
      hipLaunchKernelGGL(morph_probe_kernel<6>, g, b, 0, st, (const int4 *)in.v, (const uint32_t *)in.k, in.n, depth, erode ? 1 : 0, border, mask, cnt);
    else
      hipLaunchKernelGGL(morph_probe_kernel<26>, g, b, 0, st, (const int4 *)in.v, (const uint32_t *)in.k, in.n, depth, erode ? 1 : 0, border, mask, cnt);
  }
  // out = E_border(in), in.n > 0
  int erode(const List &in, int border, List &out) {
    DeviceScratch &S = out.mem;
    uint32_t *mask = S.get<uint32_t>(in.n), *cnt = S.get<uint32_t>((size_t)in.n + 1), *scr = S.get<uint32_t>(scan_scratch_words((size_t)in.n + 1));
    out.v = S.get<int4>(in.n); out.k = S.get<uint32_t>(in.n);
    if (!mask || !cnt || !scr || !out.v || !out.k) return fail(front, TDT_ERR_HIP, kNoMemory);
    probe(in, true, border, mask, cnt);
    if (int rc = scan_gather_count(front, st, in.v, in.k, cnt, in.n, scr, out.v, out.k, host_word)) return rc;
    out.n = *host_word;
    return TDT_OK;
  }
  // out = D(in), in.n > 0; fixed: material + 1 of every new voxel, 0 = inherit
  int dilate(const List &in, uint32_t fixed, List &out) {
    DeviceScratch &S = out.mem;
    uint32_t *mask = S.get<uint32_t>(in.n), *cnt = S.get<uint32_t>((size_t)in.n + 1), *scr = S.get<uint32_t>(scan_scratch_words((size_t)in.n + 1));
    if (!mask || !cnt || !scr) return fail(front, TDT_ERR_HIP, kNoMemory);
    probe(in, false, 0, mask, cnt);
    TDT_HIP(front, exclusive_scan_u32(st, cnt, cnt, in.n + 1u, scr));
    if (int rc = read_word(cnt + in.n)) return rc;
    const uint32_t nc = *host_word;                      // candidates: at most 26 * 2^26 < 2^32
    if (nc > kVoxelListCap) return fail(front, TDT_ERR_INVALID_VALUE, "a dilate step emits " + std::to_string(nc) + " candidate voxels (more than 2^26)");
    uint32_t nu = 0, *uk = nullptr, *uv = nullptr;
    if (nc) {
      uint32_t *ck = S.get<uint32_t>(nc), *cv = S.get<uint32_t>(nc), *ck_alt = S.get<uint32_t>(nc), *cv_alt = S.get<uint32_t>(nc);
      uint32_t *hist = S.get<uint32_t>(sort_hist_words(nc)), *hscr = S.get<uint32_t>(sort_scratch_words(nc));
      uint32_t *flag = S.get<uint32_t>((size_t)nc + 1), *fscr = S.get<uint32_t>(scan_scratch_words((size_t)nc + 1));
      if (!ck || !cv || !ck_alt || !cv_alt || !hist || !hscr || !flag || !fscr) return fail(front, TDT_ERR_HIP, kNoMemory);
      hipLaunchKernelGGL(morph_emit_kernel, dim3(blocks_of(in.n)), dim3(256), 0, st, (const int4 *)in.v, (const uint32_t *)mask, (const uint32_t *)cnt,
                         in.n, ck, cv);
      uint32_t *k = ck, *v = cv;
      TDT_HIP(front, sort_pairs_u32(st, k, v, ck_alt, cv_alt, nc, hist, hscr));
      uk = k == ck ? ck_alt : ck; uv = v == cv ? cv_alt : cv;                  // the pair the sort left free
      hipLaunchKernelGGL(morph_head_flags_kernel, dim3(blocks_of((size_t)nc + 1)), dim3(256), 0, st, (const uint32_t *)k, nc, flag);
      TDT_HIP(front, exclusive_scan_u32(st, flag, flag, nc + 1u, fscr));
      hipLaunchKernelGGL(morph_unique_kernel, dim3(blocks_of(nc)), dim3(256), 0, st, (const uint32_t *)k, (const uint32_t *)v, nc,
                         (const uint32_t *)flag, fixed, uk, uv);
      if (int rc = read_word(flag + nc)) return rc;
      nu = *host_word;
    }
    const unsigned long long total = (unsigned long long)in.n + nu;
    if (total > kVoxelListCap) return fail(front, TDT_ERR_INVALID_VALUE, "a dilate step grows the list to " + std::to_string(total) + " voxels (more than 2^26)");
    out.n = (uint32_t)total;
    out.v = S.get<int4>(out.n); out.k = S.get<uint32_t>(out.n);
    if (!out.v || !out.k) return fail(front, TDT_ERR_HIP, kNoMemory);
    hipLaunchKernelGGL(morph_merge_list_kernel, dim3(blocks_of(in.n)), dim3(256), 0, st, (const int4 *)in.v, (const uint32_t *)in.k, in.n,
                       (const uint32_t *)uk, nu, out.v, out.k);
    if (nu)
      hipLaunchKernelGGL(morph_merge_new_kernel, dim3(blocks_of(nu)), dim3(256), 0, st, (const uint32_t *)in.k, in.n, (const uint32_t *)uk,
                         (const uint32_t *)uv, nu, out.v, out.k);
    TDT_HIP(front, hipGetLastError());
    return TDT_OK;
  }
};

// what one call asks for, validated on the host before anything is queued
struct Request {
  tdt_morph m;
  std::vector<RegionShape> shapes;
};

int make_request(tdt_ctx *ctx, const tdt_morph *m, const tdt_region *regions, size_t n_regions, Request &R) {
  if (!m) return fail(ctx, TDT_ERR_INVALID_VALUE, "null tdt_morph pointer");
  if (m->op < TDT_MORPH_DILATE || m->op > TDT_MORPH_SHELL) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_MORPH_* value");
  if (m->connectivity != 6 && m->connectivity != 26) return fail(ctx, TDT_ERR_INVALID_VALUE, "connectivity must be 6 or 26");
  if (m->radius < 1 || m->radius > 64) return fail(ctx, TDT_ERR_INVALID_VALUE, "radius must be 1..64");
  if (m->material < -1 || m->material > 253) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be -1 (inherit) or 0..253");
  if (m->border != 0 && m->border != 1) return fail(ctx, TDT_ERR_INVALID_VALUE, "border must be 0 or 1");
  R.m = *m;
  return region_shapes(ctx, regions, n_regions, &R.shapes);
}

// one single-device context: the edit (n_cells) or, host_out / n_out, the result into host memory
int morph_one(tdt_ctx *front, tdt_ctx *ctx, const Request &R, uint32_t *n_cells, bool extract, int32_t *host_out, size_t capacity, size_t *n_out) {
  const tdt_morph &M = R.m;
  TDT_HIP(front, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  uint32_t word = 0;
  DeviceScratch S;                                       // V, its keys, the shapes, the combine pass
  std::unique_ptr<List> prev, cur, next;
  Drain drain{st};                                       // before anything above is freed
  int4 *v0 = nullptr;
  uint32_t nv = 0;
  int depth = 0;
  if (int rc = tree_voxels_capped(front, ctx, S, &v0, &nv, &depth)) return rc;
  const int4 *res = nullptr;
  uint32_t n_res = 0;
  if (nv) {
    uint32_t *k0 = S.get<uint32_t>(nv);
    RegionShape *d_shapes = nullptr;
    if (!k0) return fail(front, TDT_ERR_HIP, kNoMemory);
    if (int rc = upload_shapes(front, st, S, R.shapes.data(), R.shapes.size(), kNoMemory, &d_shapes)) return rc;
    voxlist_keys(st, v0, nv, k0);
    cur.reset(new List);
    cur->v = v0; cur->k = k0; cur->n = nv;               // (owned by S)
    Step T{front, ctx, st, depth, M.connectivity, &word};
    const uint32_t fixed = M.material >= 0 ? (uint32_t)M.material + 1u : 0u;
    // the two phases: r steps each
    const bool erode_first = M.op == TDT_MORPH_ERODE || M.op == TDT_MORPH_SHELL || M.op == TDT_MORPH_OPEN;
    const int phases = (M.op == TDT_MORPH_OPEN || M.op == TDT_MORPH_CLOSE) ? 2 : 1;
    const int border = phases == 2 ? 1 : M.border;
    for (int ph = 0; ph < phases; ph++) {
      const bool erode = erode_first == (ph == 0);
      for (int s = 0; s < M.radius && cur->n; s++) {     // an empty list stays empty under both steps
        next.reset(new List);
        if (int rc = erode ? T.erode(*cur, border, *next) : T.dilate(*cur, fixed, *next)) return rc;
        prev = std::move(cur);                           // the step before prev's has synchronised since: its list goes
        cur = std::move(next);
      }
    }
    res = cur->v; n_res = cur->n;
    // ---- combine with V: SHELL, OPEN, the mask ----
    const uint32_t n_shapes = (uint32_t)R.shapes.size();
    if (M.op == TDT_MORPH_SHELL || M.op == TDT_MORPH_OPEN) {
      uint32_t *keep = S.get<uint32_t>((size_t)nv + 1), *scr = S.get<uint32_t>(scan_scratch_words((size_t)nv + 1));
      int4 *out = S.get<int4>(nv);
      if (!keep || !scr || !out) return fail(front, TDT_ERR_HIP, kNoMemory);
      hipLaunchKernelGGL(morph_select_kernel, dim3(blocks_of((size_t)nv + 1)), dim3(256), 0, st, (const int4 *)v0, (const uint32_t *)k0, nv,
                         (const uint32_t *)cur->k, cur->n, M.op == TDT_MORPH_OPEN ? 1 : 0, (const RegionShape *)d_shapes, n_shapes, keep);
      if (int rc = scan_gather_count(front, st, v0, nullptr, keep, nv, scr, out, nullptr, &word)) return rc;
      res = out; n_res = word;
    } else if (n_shapes) {
      const uint32_t nr = cur->n;
      const size_t n_slots = (size_t)nr + nv;
      uint32_t *keep = S.get<uint32_t>(n_slots + 1), *scr = S.get<uint32_t>(scan_scratch_words(n_slots + 1));
      int4 *slot = S.get<int4>(n_slots), *out = S.get<int4>(n_slots);
      if (!keep || !scr || !slot || !out) return fail(front, TDT_ERR_HIP, kNoMemory);
      hipLaunchKernelGGL(morph_mask_result_kernel, dim3(blocks_of((size_t)nr + 1)), dim3(256), 0, st, (const int4 *)cur->v, (const uint32_t *)cur->k, nr,
                         (const uint32_t *)k0, nv, (const RegionShape *)d_shapes, n_shapes, slot, keep);
      hipLaunchKernelGGL(morph_mask_tree_kernel, dim3(blocks_of(nv)), dim3(256), 0, st, (const int4 *)v0, (const uint32_t *)k0, nv,
                         (const uint32_t *)cur->k, nr, (const RegionShape *)d_shapes, n_shapes, slot, keep);
      if (int rc = scan_gather_count(front, st, slot, nullptr, keep, (uint32_t)n_slots, scr, out, nullptr, &word)) return rc;
      res = out; n_res = word;
    } else {
      TDT_HIP(front, hipGetLastError());
      TDT_HIP(front, hipStreamSynchronize(st));           // a dilate step's merge may still be running
    }
    if (n_res > kVoxelListCap) return fail(front, TDT_ERR_INVALID_VALUE, "the result holds " + std::to_string(n_res) + " voxels (more than 2^26)");
  }
  if (extract) return list_to_host(front, st, res, n_res, sizeof(int4), "voxels", host_out, capacity, n_out);
  // ---- rebuild and install ----
  return rebuild_install(front, ctx, res, n_res, depth, true, n_cells, [&] { prev.reset(); cur.reset(); S.release(); });
}

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_octree_morph(tdt_ctx *ctx, const tdt_morph *m, const tdt_region *regions, size_t n_regions, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  Request R;
  if (int rc = make_request(ctx, m, regions, n_regions, R)) return rc;
  // every replica, as region edits do, a misfit reporting the size to grow to
  return edit_replicas(ctx, true, n_cells, [&](tdt_ctx *mem, uint32_t *nc) { return morph_one(ctx, mem, R, nc, false, nullptr, 0, nullptr); });
}

int tdt_octree_extract_morph(tdt_ctx *ctx, const tdt_morph *m, const tdt_region *regions, size_t n_regions, int32_t *voxels_xyzm,
                             size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  Request R;
  if (int rc = make_request(ctx, m, regions, n_regions, R)) return rc;
  return morph_one(ctx, first_member(ctx), R, nullptr, true, voxels_xyzm, capacity, n_voxels);
}

}  // extern "C"
