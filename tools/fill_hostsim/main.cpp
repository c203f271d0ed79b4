// drives the real entry points of fill_unit.cpp on lists made here, against a plain BFS
#include <algorithm>
#include <array>
#include <cstdio>
#include <queue>
#include <random>
#include "tdt_internal.hpp"
static std::vector<int4> g_list; static int g_depth;
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
int tree_voxels(tdt_ctx *, tdt_ctx *, uint32_t, DeviceScratch &S, int4 **out, uint32_t *n, int *depth) {
  *depth = g_depth; *n = (uint32_t)g_list.size(); *out = nullptr;
  if (g_list.empty()) return 0;
  *out = S.get<int4>(g_list.size()); std::memcpy(*out, g_list.data(), g_list.size() * sizeof(int4)); return 0;
}
int check_mesh(tdt_ctx *, const tdt_mesh *) { return 0; }
int mesh_voxels(tdt_ctx *f, tdt_ctx *c, const tdt_mesh *, int, DeviceScratch &S, const int4 **out, uint32_t *n) {
  int4 *o; int d; const int rc = tree_voxels(f, c, 0, S, &o, n, &d); *out = o; return rc;
}
int region_edit_source(tdt_ctx *, int, VoxelSource &, uint32_t *) { return 0; }
}
// Morton key of the library's lists: spread3(x) << 2 | spread3(y) << 1 | spread3(z)
static uint32_t key(int x, int y, int z) {
  uint32_t k = 0;
  for (int b = 0; b < 10; b++)
    k |= ((x >> b) & 1u) << (3 * b + 2) | ((y >> b) & 1u) << (3 * b + 1) | ((z >> b) & 1u) << (3 * b);
  return k;
}

// one case: the unit's list for the wall set W against a queue BFS from the grid's faces on a dense grid
static int run_case(const char *name, int depth, std::vector<int4> W, int conn, int material, bool solid) {
  const int N = 1 << depth;
  std::sort(W.begin(), W.end(), [](const int4 &a, const int4 &b) { return key(a.x, a.y, a.z) < key(b.x, b.y, b.z); });
  g_list = W;
  g_depth = depth;
  std::vector<int> mat((size_t)N * N * N, 0);              // material + 1 of the wall voxel, 0: empty
  std::vector<char> out((size_t)N * N * N, 0);             // empty and outside
  auto cell = [&](int x, int y, int z) { return ((size_t)x * N + y) * N + z; };
  for (auto &p : W) mat[cell(p.x, p.y, p.z)] = p.w;
  std::queue<std::array<int, 3>> q;
  for (int x = 0; x < N; x++)
    for (int y = 0; y < N; y++)
      for (int z = 0; z < N; z++) {
        const bool face = x == 0 || y == 0 || z == 0 || x == N - 1 || y == N - 1 || z == N - 1;
        if (face && !mat[cell(x, y, z)]) { out[cell(x, y, z)] = 1; q.push({x, y, z}); }
      }
  while (!q.empty()) {
    const auto p = q.front();
    q.pop();
    for (int dx = -1; dx <= 1; dx++)
      for (int dy = -1; dy <= 1; dy++)
        for (int dz = -1; dz <= 1; dz++) {
          const int s = std::abs(dx) + std::abs(dy) + std::abs(dz);
          if (!s || (conn == 6 && s != 1)) continue;
          const int x = p[0] + dx, y = p[1] + dy, z = p[2] + dz;
          if (x < 0 || y < 0 || z < 0 || x >= N || y >= N || z >= N) continue;
          if (out[cell(x, y, z)] || mat[cell(x, y, z)]) continue;
          out[cell(x, y, z)] = 1;
          q.push({x, y, z});
        }
  }
  // the expected list: E (and W for the solid form), materials by the -x rule, in Morton order
  std::vector<std::pair<uint32_t, int4>> want;
  for (int x = 0; x < N; x++)
    for (int y = 0; y < N; y++)
      for (int z = 0; z < N; z++) {
        if (mat[cell(x, y, z)]) {
          if (solid) want.push_back({key(x, y, z), int4{x, y, z, mat[cell(x, y, z)]}});
          continue;
        }
        if (out[cell(x, y, z)]) continue;
        int m = material + 1;
        if (material < 0) {
          int xx = x;
          while (!mat[cell(xx, y, z)]) xx--;
          m = mat[cell(xx, y, z)];
        }
        want.push_back({key(x, y, z), int4{x, y, z, m}});
      }
  std::sort(want.begin(), want.end(), [](auto &a, auto &b) { return a.first < b.first; });
  // the unit: count, then fill
  tdt_ctx ctx{};
  tdt_fill f{conn, material};
  tdt_mesh mesh{};
  size_t n = 0;
  auto call = [&](int32_t *dst, size_t capacity) {
    return solid ? tdt_voxelize_triangles_solid(&ctx, &mesh, depth, &f, dst, capacity, &n)
                 : tdt_octree_extract_enclosed(&ctx, &f, nullptr, 0, dst, capacity, &n);
  };
  int rc = call(nullptr, 0);
  std::vector<int32_t> got(4 * n + 4);
  if (!rc && n) rc = call(got.data(), n);
  bool ok = rc == 0 && n == want.size();
  for (size_t i = 0; ok && i < n; i++) {
    const int4 &w = want[i].second;
    ok = got[4 * i] == w.x && got[4 * i + 1] == w.y && got[4 * i + 2] == w.z && got[4 * i + 3] == w.w;
  }
  std::printf("%-28s depth %d conn %2d mat %3d solid %d: |W| %zu want %zu got %zu passes %d %s\n", name, depth, conn, material,
              (int)solid, W.size(), want.size(), n, tdt_debug_fill_passes(&ctx), ok ? "OK" : "MISMATCH");
  return ok ? 0 : 1;
}

// a box with walls one voxel thick, three materials by row
static std::vector<int4> hollow(int x0, int y0, int z0, int x1, int y1, int z1, int m) {
  std::vector<int4> v;
  for (int x = x0; x <= x1; x++)
    for (int y = y0; y <= y1; y++)
      for (int z = z0; z <= z1; z++)
        if (x == x0 || x == x1 || y == y0 || y == y1 || z == z0 || z == z1) v.push_back(int4{x, y, z, m + (y - y0) % 3});
  return v;
}

int main(int argc, char **argv) {
  int bad = 0;
  std::mt19937 rng(7);
  if (argc > 1) {                                          // a case file: "depth conn material solid", then "x y z m" per wall voxel
    FILE *f = std::fopen(argv[1], "r");
    int depth, conn, mat, solid;
    std::vector<int4> W;
    int4 p;
    if (!f || std::fscanf(f, "%d %d %d %d", &depth, &conn, &mat, &solid) != 4) return 2;
    while (std::fscanf(f, "%d %d %d %d", &p.x, &p.y, &p.z, &p.w) == 4) W.push_back(p);
    std::fclose(f);
    return run_case(argv[1], depth, W, conn, mat, solid != 0);
  }
  for (int depth : {3, 4, 5})
    for (int conn : {6, 26}) {
      std::vector<int4> W;
      const int N = 1 << depth;
      const unsigned density = conn == 6 ? 600 : 900;      // per mille: pockets under 26 need thick rock
      for (int x = 0; x < N; x++)
        for (int y = 0; y < N; y++)
          for (int z = 0; z < N; z++)
            if (rng() % 1000 < density) W.push_back(int4{x, y, z, 1 + (int)(rng() % 254)});
      bad += run_case("random", depth, W, conn, -1, false);
      bad += run_case("random", depth, W, conn, 17, depth == 4);
    }
  {                                                        // walls in words 0 / 1, 1 / 2 and 0 of a row at depth 7
    auto a = hollow(30, 3, 5, 34, 12, 9, 1), b = hollow(61, 20, 30, 66, 26, 33, 7), c = hollow(1, 40, 40, 3, 44, 43, 20);
    a.insert(a.end(), b.begin(), b.end());
    a.insert(a.end(), c.begin(), c.end());
    bad += run_case("boxes across words", 7, a, 6, -1, false);
    bad += run_case("boxes across words", 7, a, 26, -1, true);
    a.erase(a.begin() + 7);
    bad += run_case("one box with a hole", 7, a, 6, -1, false);
  }
  bad += run_case("empty", 4, {}, 6, -1, false);
  bad += run_case("one voxel", 4, {int4{3, 4, 5, 9}}, 26, -1, true);
  bad += run_case("plate", 4, hollow(3, 0, 2, 3, 15, 14, 3), 6, -1, false);
  std::printf(bad ? "FAILED %d\n" : "all ok\n", bad);
  return bad != 0;
}
