// Triangle-mesh voxelisation (include/tdt_rt.h tdt_voxelize_triangles / tdt_octree_edit_triangles): the voxels of the grid
// [0, 2^depth)^3 whose closed cube shares a point with a closed triangle, decided exactly in int64 by the 13-axis
// separating-axis test, each with the material of the highest-index triangle that covers it.
//
//   setup    one lane per triangle: edges, normal, the triangle's interval on each of the 9 edge x box-axis products, its
//            grid-clipped voxel range and the number of 8^3-voxel tiles that range touches.            mesh_setup_kernel
//   tiles    exclusive scan of the tile counts; one lane per (triangle, tile) finds its triangle by a binary search of the
//            scan and tests the triangle against the closed tile box; a second scan over the flags compacts the surviving
//            pairs in candidate order, which is triangle order.                         mesh_tiles_kernel, mesh_pairs_kernel
//   voxels   one wave per surviving pair walks the voxels of (tile & the triangle's voxel range), 64 per step, the triangle's
//            setup being wave-uniform.  It runs twice: a counting pass (per-pair counts + a 64-bit total the host checks
//            against the cap before anything is sized by it), then, after a scan of the counts, the emitting pass writes
//            (Morton key, triangle) at its pair's offset — so the pairs are in triangle order.              mesh_voxels_kernel
//   unique   the builder's stable radix sort keeps that order inside every run of equal keys; the last of a run is the
//            highest triangle.  Scan of the last flags, then {x, y, z, material + 1} per kept key.  mesh_last_kernel, mesh_emit_kernel
//
// Arithmetic bound (|coordinate| <= 2^18 units, 64 units per voxel, box corners in [0, 2^16], box side <= 2^9):
//   edge components           |e|  <= 2^19
//   normal n = e0 x e1        |n_k| <= 2 * 2^19 * 2^19 = 2^39
//   n . v0                    <= 3 * 2^39 * 2^18 = 3 * 2^57;  n . corner <= 3 * 2^39 * 2^16 = 3 * 2^55
//   side * sum |n_k|          <= 2^9 * 3 * 2^39 = 3 * 2^48          => every plane term stays below 2^60
//   edge x axis projections   e_w * p_u - e_u * p_w <= 2 * 2^19 * 2^18 = 2^38 (+ 2^9 * 2^20 for the box radius)
// so signed 64-bit arithmetic is exact throughout.
#include <cstring>
#include <string>
#include <vector>

#include "device_scan.hpp"
#include "region_device.hpp"
#include "tdt_internal.hpp"

namespace tdt {

constexpr int kMeshUnit = 1 << TDT_MESH_FRAC;          // units per voxel
constexpr int kMeshTile = 8;                           // voxels per tile side
constexpr unsigned long long kMeshCap = 1ull << 26;    // level-1 candidates, and covered (triangle, voxel) pairs

struct MeshTri {               // what the per-candidate test reads
  long long n[3], d0;          // normal, n . v0
  long long nneg, npos;        // sum of the negative / positive normal components
  long long tmin[9], tmax[9];  // edge i x axis k (index 3 i + k): the triangle's interval
  int32_t e[9];                // edges e[3 i + k] = (v[i + 1] - v[i])[k]
  int32_t lo[3], hi[3];        // bounding box, units
  int32_t vlo[3], vhi[3];      // voxel range inside the grid, inclusive (vhi < vlo on some axis: none)
  int32_t pad[3];
};
static_assert(sizeof(MeshTri) == 48 + 144 + 36 + 48 + 12, "MeshTri is 288 bytes");

// first / last voxel a closed interval [lo, hi] of units touches: voxel x is [64 x, 64 x + 64], so a coordinate on a
// voxel boundary touches both neighbours
__host__ __device__ inline int mesh_first_voxel(int lo) { return (lo - 1) >> TDT_MESH_FRAC; }
__host__ __device__ inline int mesh_last_voxel(int hi) { return hi >> TDT_MESH_FRAC; }

// tiles of the grid-clipped voxel range of [lo, hi] (units, per axis); 0 when the range misses the grid
__host__ __device__ inline uint32_t mesh_tile_count(const int lo[3], const int hi[3], int N, int vlo[3], int vhi[3]) {
  uint32_t n = 1;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    int f = mesh_first_voxel(lo[a]), l = mesh_last_voxel(hi[a]);
    f = f < 0 ? 0 : f; l = l > N - 1 ? N - 1 : l;
    vlo[a] = f; vhi[a] = l;
    n *= l >= f ? (uint32_t)((l >> 3) - (f >> 3) + 1) : 0u;
  }
  return n;
}

// closed triangle against the closed box [b, b + s]^3 (units): no separating axis among the 13
__device__ __forceinline__ bool mesh_overlap(const MeshTri &T, int bx, int by, int bz, int s) {
  const int b[3] = {bx, by, bz};
  if (T.hi[0] < bx || T.lo[0] > bx + s || T.hi[1] < by || T.lo[1] > by + s || T.hi[2] < bz || T.lo[2] > bz + s) return false;
  const long long d = T.n[0] * bx + T.n[1] * by + T.n[2] * bz - T.d0;      // the plane's value at the box's low corner
  if (d + T.nneg * s > 0 || d + T.npos * s < 0) return false;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int u = (k + 1) % 3, w = (k + 2) % 3;                          // axis e_i x unit_k = (.., e_w at u, -e_u at w)
      const int au = T.e[3 * i + w], aw = -T.e[3 * i + u];
      const long long p = (long long)au * b[u] + (long long)aw * b[w];
      const long long neg = (long long)(au < 0 ? au : 0) + (aw < 0 ? aw : 0), pos = (long long)(au > 0 ? au : 0) + (aw > 0 ? aw : 0);
      if (T.tmax[3 * i + k] < p + neg * s || T.tmin[3 * i + k] > p + pos * s) return false;
    }
  }
  return true;
}

__global__ __launch_bounds__(256) void mesh_setup_kernel(const int32_t *vtx, const uint32_t *idx, const int32_t *mats, int32_t material1,
                                                        uint32_t n_tri, int N, MeshTri *tris, uint32_t *mat, uint32_t *count) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t > n_tri) return;
  if (t == n_tri) { count[t] = 0; return; }                  // the scan's extra item: its slot receives the total
  int v[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) v[i][k] = vtx[3 * (size_t)idx[3 * (size_t)t + i] + k];
  MeshTri T;
#pragma unroll
  for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) T.e[3 * i + k] = v[(i + 1) % 3][k] - v[i][k];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int u = (k + 1) % 3, w = (k + 2) % 3;
    T.n[k] = (long long)T.e[u] * T.e[3 + w] - (long long)T.e[w] * T.e[3 + u];          // e0 x e1
    int lo = v[0][k], hi = v[0][k];
#pragma unroll
    for (int i = 1; i < 3; i++) { lo = v[i][k] < lo ? v[i][k] : lo; hi = v[i][k] > hi ? v[i][k] : hi; }
    T.lo[k] = lo; T.hi[k] = hi;
  }
  T.d0 = T.n[0] * v[0][0] + T.n[1] * v[0][1] + T.n[2] * v[0][2];
  T.nneg = T.npos = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) { if (T.n[k] < 0) T.nneg += T.n[k]; else T.npos += T.n[k]; }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int u = (k + 1) % 3, w = (k + 2) % 3;
      const long long au = T.e[3 * i + w], aw = -(long long)T.e[3 * i + u];
      long long lo = 0, hi = 0;
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const long long p = au * v[j][u] + aw * v[j][w];
        lo = (j == 0 || p < lo) ? p : lo; hi = (j == 0 || p > hi) ? p : hi;
      }
      T.tmin[3 * i + k] = lo; T.tmax[3 * i + k] = hi;
    }
  T.pad[0] = T.pad[1] = T.pad[2] = 0;
  count[t] = mesh_tile_count(T.lo, T.hi, N, T.vlo, T.vhi);
  tris[t] = T;
  mat[t] = (uint32_t)(mats ? mats[t] : material1);
}

// the triangle of candidate g: the last one whose first candidate is <= g (a triangle without candidates shares its
// successor's first candidate, so it is never the last)
__device__ __forceinline__ uint32_t mesh_find_triangle(const uint32_t *first, uint32_t n_tri, uint32_t g) {
  uint32_t lo = 0, hi = n_tri;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (first[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}

// tile (in tiles) of candidate l of triangle T
__device__ __forceinline__ void mesh_tile_of(const MeshTri &T, uint32_t l, int tile[3]) {
  const uint32_t ey = (uint32_t)((T.vhi[1] >> 3) - (T.vlo[1] >> 3) + 1), ez = (uint32_t)((T.vhi[2] >> 3) - (T.vlo[2] >> 3) + 1);
  tile[0] = (T.vlo[0] >> 3) + (int)(l / (ey * ez));
  tile[1] = (T.vlo[1] >> 3) + (int)((l / ez) % ey);
  tile[2] = (T.vlo[2] >> 3) + (int)(l % ez);
}

__global__ __launch_bounds__(256) void mesh_tiles_kernel(const MeshTri *tris, const uint32_t *first, uint32_t n_tri, uint32_t n_cand, uint32_t *flag) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g > n_cand) return;
  if (g == n_cand) { flag[g] = 0; return; }
  const uint32_t t = mesh_find_triangle(first, n_tri, g);
  const MeshTri &T = tris[t];
  int tile[3];
  mesh_tile_of(T, g - first[t], tile);
  const int s = kMeshTile * kMeshUnit;
  flag[g] = mesh_overlap(T, tile[0] * s, tile[1] * s, tile[2] * s, s) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void mesh_pairs_kernel(const MeshTri *tris, const uint32_t *first, uint32_t n_tri, uint32_t n_cand,
                                                        const uint32_t *excl, uint2 *pairs) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_cand || excl[g + 1u] == excl[g]) return;
  const uint32_t t = mesh_find_triangle(first, n_tri, g);
  int tile[3];
  mesh_tile_of(tris[t], g - first[t], tile);
  pairs[excl[g]] = make_uint2(t, (uint32_t)tile[0] | ((uint32_t)tile[1] << 7) | ((uint32_t)tile[2] << 14));
}

// one wave per pair.  EMIT false: counts[p] = covered voxels, *total += them.  EMIT true: the pairs at offset[p].
// The pair is wave-uniform, so its triangle sits in scalar registers, and the test is mesh_overlap's rewritten relative to the
// tile's low corner o: a candidate's corner is o + l with 0 <= l <= 448 units, so an edge axis a gives a . l, |a . l| <=
// 2 * 2^19 * 448 < 2^29, in 32 bits (operands of 21 and 9 bits), against thresholds tmax - a . o - 64 neg and tmin - a . o -
// 64 pos folded once per wave and clamped to +-2^30, which no a . l reaches, so the clamp changes no comparison.  The plane
// keeps 64 bits: n . l with |n_k| <= 2^39.
template <bool EMIT>
__global__ __launch_bounds__(256) void mesh_voxels_kernel(const MeshTri *tris, const uint2 *pairs, uint32_t n_pairs, uint32_t *counts,
                                                         unsigned long long *total, const uint32_t *offset, uint32_t *keys, uint32_t *vals) {
  const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (p >= n_pairs) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint2 pr = pairs[p];
  const MeshTri &T = tris[pr.x];
  int org[3], lo[3], ext[3];                                  // tile origin, first candidate, candidates per axis (voxels)
#pragma unroll
  for (int a = 0; a < 3; a++) {
    org[a] = (int)((pr.y >> (7 * a)) & 127u) * kMeshTile;
    const int f = T.vlo[a] > org[a] ? T.vlo[a] : org[a], l = T.vhi[a] < org[a] + kMeshTile - 1 ? T.vhi[a] : org[a] + kMeshTile - 1;
    lo[a] = f; ext[a] = l - f + 1;                            // >= 1: the tile lies in the triangle's tile range
  }
  constexpr long long kClamp = 1ll << 30;
  int au[9], aw[9], thi[9], tlo[9];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int u = (k + 1) % 3, w = (k + 2) % 3, j = 3 * i + k;
      au[j] = T.e[3 * i + w]; aw[j] = -T.e[3 * i + u];
      const long long o = ((long long)au[j] * org[u] + (long long)aw[j] * org[w]) * kMeshUnit;
      const long long neg = (long long)(au[j] < 0 ? au[j] : 0) + (aw[j] < 0 ? aw[j] : 0), pos = (long long)(au[j] > 0 ? au[j] : 0) + (aw[j] > 0 ? aw[j] : 0);
      const long long h = T.tmax[j] - o - neg * kMeshUnit, l = T.tmin[j] - o - pos * kMeshUnit;
      thi[j] = (int)(h > kClamp ? kClamp : h < -kClamp ? -kClamp : h);
      tlo[j] = (int)(l > kClamp ? kClamp : l < -kClamp ? -kClamp : l);
    }
  }
  const long long d_org = (T.n[0] * org[0] + T.n[1] * org[1] + T.n[2] * org[2]) * kMeshUnit - T.d0;
  const long long dlo = d_org + T.nneg * kMeshUnit, dhi = d_org + T.npos * kMeshUnit;
  const uint32_t cand = (uint32_t)(ext[0] * ext[1] * ext[2]);
  const uint32_t base = EMIT ? offset[p] : 0u;
  uint32_t done = 0;
  for (uint32_t c0 = 0; c0 < cand; c0 += 64u) {
    const uint32_t c = c0 + lane;
    bool hit = false;
    int x = 0, y = 0, z = 0;
    if (c < cand) {
      x = lo[0] + (int)(c / (uint32_t)(ext[1] * ext[2]));
      y = lo[1] + (int)((c / (uint32_t)ext[2]) % (uint32_t)ext[1]);
      z = lo[2] + (int)(c % (uint32_t)ext[2]);
      const int b[3] = {x * kMeshUnit, y * kMeshUnit, z * kMeshUnit};
      const int l[3] = {(x - org[0]) * kMeshUnit, (y - org[1]) * kMeshUnit, (z - org[2]) * kMeshUnit};
      hit = !(T.hi[0] < b[0] || T.lo[0] > b[0] + kMeshUnit || T.hi[1] < b[1] || T.lo[1] > b[1] + kMeshUnit || T.hi[2] < b[2] ||
              T.lo[2] > b[2] + kMeshUnit);
      const long long nl = T.n[0] * l[0] + T.n[1] * l[1] + T.n[2] * l[2];
      hit = hit && !(dlo + nl > 0 || dhi + nl < 0);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int u = (k + 1) % 3, w = (k + 2) % 3;
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const int q = au[3 * i + k] * l[u] + aw[3 * i + k] * l[w];
          hit = hit && !(thi[3 * i + k] < q || tlo[3 * i + k] > q);
        }
      }
    }
    const unsigned long long ball = __ballot(hit);
    if (EMIT && hit) {
      const uint32_t pos = base + done + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
      keys[pos] = region_key(x, y, z); vals[pos] = pr.x;
    }
    done += (uint32_t)__popcll(ball);
  }
  if (!EMIT && lane == 0) { counts[p] = done; if (done) atomicAdd(total, (unsigned long long)done); }
}

// of every run of equal sorted keys the last (the stable sort kept triangle order); flag[n] = 0
__global__ __launch_bounds__(256) void mesh_last_kernel(const uint32_t *keys, uint32_t n, uint32_t *flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  flag[i] = (i < n && (i + 1u == n || keys[i + 1u] != keys[i])) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void mesh_emit_kernel(const uint32_t *keys, const uint32_t *tri, uint32_t n, const uint32_t *excl,
                                                       const uint32_t *mat, int4 *out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || excl[i + 1u] == excl[i]) return;
  out[excl[i]] = region_voxel(keys[i], (int)mat[tri[i]]);
}

namespace {

const char *kNoMemory = "out of device memory in the mesh voxelisation";

// level-1 candidates of the whole mesh on a grid of side 2^depth (what mesh_setup_kernel's counts sum to)
unsigned long long tile_candidates(const tdt_mesh *m, int depth) {
  unsigned long long total = 0;
  for (size_t t = 0; t < m->n_triangles; t++) {
    int lo[3], hi[3], vlo[3], vhi[3];
    for (int k = 0; k < 3; k++) {
      lo[k] = hi[k] = m->vertices[3 * (size_t)m->triangles[3 * t] + k];
      for (int i = 1; i < 3; i++) {
        const int c = m->vertices[3 * (size_t)m->triangles[3 * t + i] + k];
        lo[k] = c < lo[k] ? c : lo[k]; hi[k] = c > hi[k] ? c : hi[k];
      }
    }
    total += mesh_tile_count(lo, hi, 1 << depth, vlo, vhi);
  }
  return total;
}

}  // namespace

// everything about a mesh that does not depend on the grid, checked on the host before anything is queued (tdt_internal.hpp)
int check_mesh(tdt_ctx *ctx, const tdt_mesh *m) {
  if (!m) return fail(ctx, TDT_ERR_INVALID_VALUE, "null mesh");
  if (m->n_triangles && !m->triangles) return fail(ctx, TDT_ERR_INVALID_VALUE, "null triangle array");
  if (m->n_vertices && !m->vertices) return fail(ctx, TDT_ERR_INVALID_VALUE, "null vertex array");
  if (!m->materials && (m->material < 0 || m->material > 253)) return fail(ctx, TDT_ERR_INVALID_VALUE, "material must be 0..253");
  for (size_t t = 0; t < m->n_triangles; t++) {
    for (int i = 0; i < 3; i++)
      if (m->triangles[3 * t + i] >= m->n_vertices)
        return fail(ctx, TDT_ERR_INVALID_VALUE, "triangle " + std::to_string(t) + ": vertex index " + std::to_string(m->triangles[3 * t + i]) +
                                                    " >= " + std::to_string(m->n_vertices) + " vertices");
    if (m->materials && (m->materials[t] < 1 || m->materials[t] > 254))
      return fail(ctx, TDT_ERR_INVALID_VALUE, "triangle " + std::to_string(t) + ": material + 1 must be 1..254");
  }
  for (size_t i = 0; i < 3 * (size_t)m->n_vertices; i++)
    if (m->vertices[i] > TDT_MESH_COORD_MAX || m->vertices[i] < -TDT_MESH_COORD_MAX)
      return fail(ctx, TDT_ERR_INVALID_VALUE, "vertex " + std::to_string(i / 3) + ": a coordinate beyond +-2^18 units");
  return TDT_OK;
}

// the mesh's voxels {x, y, z, material + 1}, Morton-sorted and unique, in device memory of ctx (allocated in S; null when
// *n == 0).  The mesh has passed check_mesh.  Queued on ctx's stream, so ordered after the work already there; synchronises.
// (tdt_internal.hpp: the solid forms of tdt_fill.hip start from this list)
int mesh_voxels(tdt_ctx *front, tdt_ctx *ctx, const tdt_mesh *m, int depth, DeviceScratch &S, const int4 **out, uint32_t *n) {
  *out = nullptr; *n = 0;
  const uint32_t nt = m->n_triangles;
  if (nt == 0) return TDT_OK;
  const unsigned long long cand64 = tile_candidates(m, depth);
  if (cand64 > kMeshCap)
    return fail(front, TDT_ERR_INVALID_VALUE, "the mesh enumerates " + std::to_string(cand64) + " candidate tiles (more than 2^26)");
  if (cand64 == 0) return TDT_OK;                          // nothing of it in the grid
  const uint32_t nc = (uint32_t)cand64;
  hipStream_t st = ctx->stream;
  // ---- setup ----
  int32_t *d_vtx = S.get<int32_t>(3 * (size_t)m->n_vertices), *d_mats = m->materials ? S.get<int32_t>(nt) : nullptr;
  uint32_t *d_idx = S.get<uint32_t>(3 * (size_t)nt), *mat = S.get<uint32_t>(nt);
  MeshTri *tris = S.get<MeshTri>(nt);
  uint32_t *first = S.get<uint32_t>((size_t)nt + 1), *scr1 = S.get<uint32_t>(scan_scratch_words((size_t)nt + 1));
  uint32_t *flag = S.get<uint32_t>((size_t)nc + 1), *scr2 = S.get<uint32_t>(scan_scratch_words((size_t)nc + 1));
  unsigned long long *d_total = S.get<unsigned long long>(1);
  if (!d_vtx || (m->materials && !d_mats) || !d_idx || !mat || !tris || !first || !scr1 || !flag || !scr2 || !d_total)
    return fail(front, TDT_ERR_HIP, kNoMemory);
  TDT_HIP(front, hipMemcpyAsync(d_vtx, m->vertices, 3 * (size_t)m->n_vertices * sizeof(int32_t), hipMemcpyHostToDevice, st));
  TDT_HIP(front, hipMemcpyAsync(d_idx, m->triangles, 3 * (size_t)nt * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (d_mats) TDT_HIP(front, hipMemcpyAsync(d_mats, m->materials, (size_t)nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
  TDT_HIP(front, hipMemsetAsync(d_total, 0, sizeof *d_total, st));
  hipLaunchKernelGGL(mesh_setup_kernel, dim3(blocks_of((size_t)nt + 1)), dim3(256), 0, st, (const int32_t *)d_vtx, (const uint32_t *)d_idx,
                     (const int32_t *)d_mats, m->material + 1, nt, 1 << depth, tris, mat, first);
  TDT_HIP(front, exclusive_scan_u32(st, first, first, nt + 1u, scr1));
  // ---- tiles ----
  hipLaunchKernelGGL(mesh_tiles_kernel, dim3(blocks_of((size_t)nc + 1)), dim3(256), 0, st, (const MeshTri *)tris, (const uint32_t *)first, nt, nc, flag);
  TDT_HIP(front, exclusive_scan_u32(st, flag, flag, nc + 1u, scr2));
  uint32_t np = 0;
  if (int rc = read_word(front, st, flag + nc, &np)) return rc;   // the surviving pairs
  if (np == 0) return TDT_OK;
  uint2 *pairs = S.get<uint2>(np);
  uint32_t *counts = S.get<uint32_t>((size_t)np + 1), *scr3 = S.get<uint32_t>(scan_scratch_words((size_t)np + 1));
  if (!pairs || !counts || !scr3) return fail(front, TDT_ERR_HIP, kNoMemory);
  hipLaunchKernelGGL(mesh_pairs_kernel, dim3(blocks_of(nc)), dim3(256), 0, st, (const MeshTri *)tris, (const uint32_t *)first, nt, nc,
                     (const uint32_t *)flag, pairs);
  // ---- voxels: count, then emit ----
  const unsigned waves = (np + 3u) / 4u;
  TDT_HIP(front, hipMemsetAsync(counts + np, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(mesh_voxels_kernel<false>, dim3(waves), dim3(256), 0, st, (const MeshTri *)tris, (const uint2 *)pairs, np, counts, d_total,
                     (const uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr);
  TDT_HIP(front, hipGetLastError());
  unsigned long long covered = 0;
  TDT_HIP(front, hipMemcpyAsync(&covered, d_total, sizeof covered, hipMemcpyDeviceToHost, st));
  TDT_HIP(front, hipStreamSynchronize(st));                // the covered (triangle, voxel) pairs
  if (covered > kMeshCap)
    return fail(front, TDT_ERR_INVALID_VALUE, "the mesh covers " + std::to_string(covered) + " (triangle, voxel) pairs (more than 2^26)");
  if (covered == 0) return TDT_OK;                         // (a surviving tile may hold no covered voxel)
  const uint32_t nk = (uint32_t)covered;
  uint32_t *k0 = S.get<uint32_t>(nk), *v0 = S.get<uint32_t>(nk), *k1 = S.get<uint32_t>(nk), *v1 = S.get<uint32_t>(nk);
  uint32_t *hist = S.get<uint32_t>(sort_hist_words(nk)), *hscr = S.get<uint32_t>(sort_scratch_words(nk));
  uint32_t *last = S.get<uint32_t>((size_t)nk + 1), *scr4 = S.get<uint32_t>(scan_scratch_words((size_t)nk + 1));
  int4 *vox = S.get<int4>(nk);
  if (!k0 || !v0 || !k1 || !v1 || !hist || !hscr || !last || !scr4 || !vox) return fail(front, TDT_ERR_HIP, kNoMemory);
  TDT_HIP(front, exclusive_scan_u32(st, counts, counts, np + 1u, scr3));
  hipLaunchKernelGGL(mesh_voxels_kernel<true>, dim3(waves), dim3(256), 0, st, (const MeshTri *)tris, (const uint2 *)pairs, np, (uint32_t *)nullptr,
                     (unsigned long long *)nullptr, (const uint32_t *)counts, k0, v0);
  // ---- sort, last of each run, materials ----
  uint32_t *k = k0, *v = v0;
  TDT_HIP(front, sort_pairs_u32(st, k, v, k1, v1, nk, hist, hscr));
  hipLaunchKernelGGL(mesh_last_kernel, dim3(blocks_of((size_t)nk + 1)), dim3(256), 0, st, (const uint32_t *)k, nk, last);
  TDT_HIP(front, exclusive_scan_u32(st, last, last, nk + 1u, scr4));
  hipLaunchKernelGGL(mesh_emit_kernel, dim3(blocks_of(nk)), dim3(256), 0, st, (const uint32_t *)k, (const uint32_t *)v, nk, (const uint32_t *)last,
                     (const uint32_t *)mat, vox);
  TDT_HIP(front, hipGetLastError());
  uint32_t nu = 0;
  if (int rc = read_word(front, st, last + nk, &nu)) return rc;   // the voxel count
  *out = vox; *n = nu;
  return TDT_OK;
}

namespace {

struct MeshSource final : VoxelSource {
  const tdt_mesh *mesh;
  explicit MeshSource(const tdt_mesh *m) : mesh(m) {}
  int run(tdt_ctx *front, tdt_ctx *ctx, int depth, DeviceScratch &S, const int4 **vox, uint32_t *n) override {
    return mesh_voxels(front, ctx, mesh, depth, S, vox, n);
  }
};

}  // namespace
}  // namespace tdt

extern "C" {

int tdt_voxelize_triangles(tdt_ctx *ctx, const tdt_mesh *mesh, int depth, int32_t *voxels_xyzm, size_t capacity, size_t *n_voxels) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (!n_voxels) return fail(ctx, TDT_ERR_INVALID_VALUE, "null n_voxels pointer");
  *n_voxels = 0;
  if (depth < 1 || depth > 10) return fail(ctx, TDT_ERR_INVALID_VALUE, "depth must be 1..10");
  if (int rc = check_mesh(ctx, mesh)) return rc;
  MeshSource src(mesh);
  return region_extract_source(ctx, src, depth, voxels_xyzm, capacity, n_voxels);
}

int tdt_octree_edit_triangles(tdt_ctx *ctx, int op, const tdt_mesh *mesh, uint32_t *n_cells) {
  using namespace tdt;
  if (!ctx) return TDT_ERR_INVALID_VALUE;
  if (op < TDT_REGION_SET || op > TDT_REGION_CLEAR) return fail(ctx, TDT_ERR_INVALID_VALUE, "op must be a TDT_REGION_* value");
  if (int rc = check_mesh(ctx, mesh)) return rc;
  MeshSource src(mesh);
  return region_edit_source(ctx, op, src, n_cells);
}

}  // extern "C"
