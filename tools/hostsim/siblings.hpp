// what the stand-in programs share: the pieces of the sibling units a bit-volume unit calls (the slot check, the tree's voxel
// list, the sort, the mesh's list, the edit that takes the source's list) and the helpers of the brute-force models
#pragma once
#include <algorithm>
#include <cstdio>
#include <random>
#include "tdt_internal.hpp"
static std::vector<int4> g_list; static int g_depth;       // the bound tree: its Morton-sorted voxels and max_depth
static std::vector<int4> g_edit; static int g_edit_op;     // the edit form: the list it handed on and the op it would be applied with
namespace tdt {
int fail(tdt_ctx *c, int code, const std::string &m) { c->err = m; std::fprintf(stderr, "fail: %s\n", m.c_str()); return code; }
int hip_fail(tdt_ctx *c, hipError_t, const char *w) { return fail(c, TDT_ERR_HIP, w); }
tdt_ctx *multi_first_member(tdt_ctx *f) { return f; }
size_t sort_hist_words(uint32_t) { return 1; }
size_t sort_scratch_words(uint32_t) { return 1; }
hipError_t sort_pairs_u32(hipStream_t, uint32_t *&k, uint32_t *&v, uint32_t *, uint32_t *, uint32_t n, uint32_t *, uint32_t *) {
  std::vector<std::pair<uint32_t, uint32_t>> p(n);
  for (uint32_t i = 0; i < n; i++) p[i] = {k[i], v[i]};
  std::stable_sort(p.begin(), p.end(), [](auto &a, auto &b) { return a.first < b.first; });
  for (uint32_t i = 0; i < n; i++) { k[i] = p[i].first; v[i] = p[i].second; }
  return 0;
}
int walk_inputs(tdt_ctx *, tdt_ctx *, int *depth) { *depth = g_depth; return 0; }
int tree_voxels(tdt_ctx *, tdt_ctx *, uint32_t, DeviceScratch &S, int4 **out, uint32_t *n, int *depth) {
  *depth = g_depth; *n = (uint32_t)g_list.size(); *out = nullptr;
  if (g_list.empty()) return 0;
  *out = S.get<int4>(g_list.size()); std::memcpy(*out, g_list.data(), g_list.size() * sizeof(int4)); return 0;
}
int check_mesh(tdt_ctx *, const tdt_mesh *) { return 0; }
int mesh_voxels(tdt_ctx *f, tdt_ctx *c, const tdt_mesh *, int, DeviceScratch &S, const int4 **out, uint32_t *n) {
  int4 *o; int d; const int rc = tree_voxels(f, c, 0, S, &o, n, &d); *out = o; return rc;
}
int region_edit_source(tdt_ctx *c, int op, VoxelSource &src, uint32_t *) {
  DeviceScratch S;
  const int4 *v = nullptr; uint32_t n = 0;
  g_edit.clear(); g_edit_op = op;
  if (int rc = src.run(c, c, g_depth, S, &v, &n)) return rc;
  g_edit.assign(v, v + n);
  return 0;
}
}
// Morton key of the library's lists: spread3(x) << 2 | spread3(y) << 1 | spread3(z)
inline uint32_t key(int x, int y, int z) {
  uint32_t k = 0;
  for (int b = 0; b < 10; b++)
    k |= ((x >> b) & 1u) << (3 * b + 2) | ((y >> b) & 1u) << (3 * b + 1) | ((z >> b) & 1u) << (3 * b);
  return k;
}
inline std::vector<int4> morton_sorted(std::vector<int4> v) {
  std::stable_sort(v.begin(), v.end(), [](const int4 &a, const int4 &b) { return key(a.x, a.y, a.z) < key(b.x, b.y, b.z); });
  return v;
}

struct Grid {
  int N;
  std::vector<int> m;            // material + 1, 0: empty; [x][y][z]
  explicit Grid(int n) : N(n), m((size_t)n * n * n, 0) {}
  size_t cell(int x, int y, int z) const { return ((size_t)x * N + y) * N + z; }
  int &at(int x, int y, int z) { return m[cell(x, y, z)]; }
  int get(int x, int y, int z) const { return m[cell(x, y, z)]; }
  bool in(int x, int y, int z) const { return x >= 0 && y >= 0 && z >= 0 && x < N && y < N && z < N; }
};
inline bool region_has(const tdt_region &r, long x, long y, long z) {
  if (r.shape == TDT_SHAPE_BOX) return x >= r.a[0] && x <= r.b[0] && y >= r.a[1] && y <= r.b[1] && z >= r.a[2] && z <= r.b[2];
  const long dx = x - r.a[0], dy = y - r.a[1], dz = z - r.a[2];
  return dx * dx + dy * dy + dz * dz <= (long)r.b[0] * r.b[0];
}
inline std::vector<int4> sorted_list(const Grid &g) {
  std::vector<int4> v;
  for (int x = 0; x < g.N; x++) for (int y = 0; y < g.N; y++) for (int z = 0; z < g.N; z++)
    if (g.get(x, y, z)) v.push_back(int4{x, y, z, g.get(x, y, z)});
  return morton_sorted(v);
}
inline bool same(const std::vector<int4> &a, const std::vector<int4> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) if (a[i].x != b[i].x || a[i].y != b[i].y || a[i].z != b[i].z || a[i].w != b[i].w) return false;
  return true;
}
// a unit's two-call extract form (count, then fill) as a list
template <class Call> int extract_list(Call call, std::vector<int4> &out) {
  size_t n = 0;
  int rc = call((int32_t *)nullptr, (size_t)0, &n);
  std::vector<int32_t> got(4 * n + 4);
  if (!rc && n) rc = call(got.data(), n, &n);
  out.resize(n);
  for (size_t i = 0; i < n; i++) out[i] = int4{got[4 * i], got[4 * i + 1], got[4 * i + 2], got[4 * i + 3]};
  return rc;
}
