// enclosed space: drives the real entry points of tdt_fill.hip on lists made here, against a plain BFS
#include <array>
#include <queue>
#include "siblings.hpp"

// one case: the unit's list for the wall set W against a queue BFS from the grid's faces on a dense grid
static int run_case(const char *name, int depth, std::vector<int4> W, int conn, int material, bool solid) {
  const int N = 1 << depth;
  g_list = W = morton_sorted(W);
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
  std::vector<int4> want;
  for (int x = 0; x < N; x++)
    for (int y = 0; y < N; y++)
      for (int z = 0; z < N; z++) {
        if (mat[cell(x, y, z)]) {
          if (solid) want.push_back(int4{x, y, z, mat[cell(x, y, z)]});
          continue;
        }
        if (out[cell(x, y, z)]) continue;
        int m = material + 1;
        if (material < 0) {
          int xx = x;
          while (!mat[cell(xx, y, z)]) xx--;
          m = mat[cell(xx, y, z)];
        }
        want.push_back(int4{x, y, z, m});
      }
  want = morton_sorted(want);
  // the unit: count, then fill
  tdt_ctx ctx{};
  tdt_fill f{conn, material};
  tdt_mesh mesh{};
  std::vector<int4> got;
  const int rc = extract_list([&](int32_t *dst, size_t capacity, size_t *n) {
    return solid ? tdt_voxelize_triangles_solid(&ctx, &mesh, depth, &f, dst, capacity, n)
                 : tdt_octree_extract_enclosed(&ctx, &f, nullptr, 0, dst, capacity, n);
  }, got);
  const size_t n = got.size();
  const bool ok = rc == 0 && same(got, want);
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
