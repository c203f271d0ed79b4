// geodesic distance: drives the real entry points of tdt_geodesic.hip on lists made here, against a brute-force Dijkstra on a
// dense grid
#include <array>
#include <queue>
#include "siblings.hpp"

struct Case {
  const char *name;
  int depth;
  tdt_geodesic q;
  std::vector<std::array<int, 3>> seeds;
  std::vector<tdt_region> mask;
  bool masked;
  std::array<int, 3> goal;
  size_t min_reach, min_passes;  // the case must not be vacuous
  bool all_forms = false;        // also the edit form and the count-only path (each one more relaxation of 256 real threads a block)
};

static int run(const Grid &g, const Case &c) {
  const int N = g.N;
  const std::vector<int4> list = sorted_list(g);
  g_list = list; g_depth = c.depth;
  // ---- the brute force: P, then a heap Dijkstra over the 26 offsets ----
  std::vector<char> P((size_t)N * N * N, 0);
  for (int x = 0; x < N; x++) for (int y = 0; y < N; y++) for (int z = 0; z < N; z++) {
    const int m = g.get(x, y, z);
    bool in = c.q.medium == TDT_MEDIUM_EMPTY ? m == 0 : (m != 0 && (c.q.match < 0 || m == c.q.match + 1));
    if (in && c.masked) { in = false; for (auto &r : c.mask) in = in || region_has(r, x, y, z); }
    P[g.cell(x, y, z)] = in;
  }
  const long INF = 1l << 40;
  std::vector<long> d((size_t)N * N * N, INF);
  typedef std::pair<long, std::array<int, 3>> Item;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  for (auto &s : c.seeds) {
    if (s[0] < 0 || s[1] < 0 || s[2] < 0 || s[0] >= N || s[1] >= N || s[2] >= N || !P[g.cell(s[0], s[1], s[2])]) continue;
    d[g.cell(s[0], s[1], s[2])] = 0; heap.push({0, s});
  }
  while (!heap.empty()) {
    const Item it = heap.top(); heap.pop();
    const auto p = it.second;
    if (it.first != d[g.cell(p[0], p[1], p[2])]) continue;
    for (int dx = -1; dx <= 1; dx++) for (int dy = -1; dy <= 1; dy++) for (int dz = -1; dz <= 1; dz++) {
      const int k = std::abs(dx) + std::abs(dy) + std::abs(dz) - 1;
      if (k < 0 || c.q.w[k] <= 0) continue;
      const int x = p[0] + dx, y = p[1] + dy, z = p[2] + dz;
      if (x < 0 || y < 0 || z < 0 || x >= N || y >= N || z >= N || !P[g.cell(x, y, z)]) continue;
      if (it.first + c.q.w[k] < d[g.cell(x, y, z)]) { d[g.cell(x, y, z)] = it.first + c.q.w[k]; heap.push({it.first + c.q.w[k], {x, y, z}}); }
    }
  }
  auto reached = [&](int x, int y, int z) { return d[g.cell(x, y, z)] <= c.q.max_cost; };
  std::vector<int4> want;
  for (int x = 0; x < N; x++) for (int y = 0; y < N; y++) for (int z = 0; z < N; z++)
    if (reached(x, y, z)) want.push_back(int4{x, y, z, c.q.material >= 0 ? c.q.material + 1 : g.get(x, y, z)});
  want = morton_sorted(want);
  std::vector<std::array<int, 3>> want_path;
  long want_cost = -1;
  {
    std::array<int, 3> p = c.goal;
    const bool in = p[0] >= 0 && p[1] >= 0 && p[2] >= 0 && p[0] < N && p[1] < N && p[2] < N;
    if (in && reached(p[0], p[1], p[2])) {
      want_cost = d[g.cell(p[0], p[1], p[2])];
      want_path.push_back(p);
      while (d[g.cell(p[0], p[1], p[2])] > 0) {
        bool moved = false;
        for (int t = 0; t < 27 && !moved; t++) {
          const int dx = t / 9 - 1, dy = (t / 3) % 3 - 1, dz = t % 3 - 1, k = std::abs(dx) + std::abs(dy) + std::abs(dz) - 1;
          if (k < 0 || c.q.w[k] <= 0) continue;
          const int x = p[0] + dx, y = p[1] + dy, z = p[2] + dz;
          if (x < 0 || y < 0 || z < 0 || x >= N || y >= N || z >= N || !P[g.cell(x, y, z)]) continue;
          if (d[g.cell(x, y, z)] + c.q.w[k] == d[g.cell(p[0], p[1], p[2])]) { p = {x, y, z}; moved = true; }
        }
        if (!moved) return 1;
        want_path.push_back(p);
      }
    }
  }
  // ---- the unit ----
  tdt_ctx ctx{};
  std::vector<int32_t> seeds;
  for (auto &s : c.seeds) seeds.insert(seeds.end(), s.begin(), s.end());
  const tdt_region *regions = c.masked ? c.mask.data() : nullptr;
  const size_t n_regions = c.masked ? c.mask.size() : 0, n_seeds = c.seeds.size();
  const size_t cells = (size_t)N * N * N;
  bool ok = true;
  {                                                        // the field over the whole grid
    const int32_t lo[3] = {0, 0, 0}, hi[3] = {N - 1, N - 1, N - 1};
    std::vector<int32_t> f(cells, 12345);
    size_t n = 0;
    const int rc = tdt_octree_geodesic_field(&ctx, &c.q, seeds.data(), n_seeds, regions, n_regions, lo, hi, f.data(), cells, &n);
    ok = ok && rc == 0 && n == cells;
    for (int x = 0; ok && x < N; x++) for (int y = 0; y < N; y++) for (int z = 0; z < N; z++)
      ok = ok && f[((size_t)z * N + y) * N + x] == (reached(x, y, z) ? (int32_t)d[g.cell(x, y, z)] : -1);
  }
  const int passes = tdt_debug_geodesic_passes(&ctx);
  const bool field_ok = ok;
  {                                                        // the list, in one call with room for the grid
    std::vector<int32_t> got(4 * cells);
    size_t n = 0;
    const int rc = tdt_octree_extract_geodesic(&ctx, &c.q, seeds.data(), n_seeds, regions, n_regions, got.data(), cells, &n);
    std::vector<int4> gl(n);
    for (size_t i = 0; i < n; i++) gl[i] = int4{got[4 * i], got[4 * i + 1], got[4 * i + 2], got[4 * i + 3]};
    ok = ok && rc == 0 && same(gl, want);
  }
  const bool list_ok = ok;
  if (c.all_forms) {                                       // the edit form hands the same list on
    uint32_t nc = 0;
    const int rc = tdt_octree_edit_geodesic(&ctx, TDT_REGION_PAINT, &c.q, seeds.data(), n_seeds, regions, n_regions, &nc);
    ok = ok && rc == 0 && g_edit_op == TDT_REGION_PAINT && same(g_edit, want);
  }
  {                                                        // the path: with room for the longest, then count-only
    std::vector<int32_t> got(3 * cells);
    size_t n = 0, n2 = 0;
    int32_t cost = 0, cost2 = 0;
    const int32_t goal[3] = {c.goal[0], c.goal[1], c.goal[2]};
    int rc = tdt_octree_geodesic_path(&ctx, &c.q, seeds.data(), n_seeds, regions, n_regions, goal, got.data(), cells, &n, &cost);
    ok = ok && rc == 0 && n == want_path.size() && cost == want_cost;
    for (size_t i = 0; ok && i < n; i++) ok = got[3 * i] == want_path[i][0] && got[3 * i + 1] == want_path[i][1] && got[3 * i + 2] == want_path[i][2];
    if (c.all_forms) {
      rc = tdt_octree_geodesic_path(&ctx, &c.q, seeds.data(), n_seeds, regions, n_regions, goal, nullptr, 0, &n2, &cost2);
      ok = ok && rc == 0 && n2 == n && cost2 == cost;
      if (n > 1) {                                         // a capacity below the count: the error, with the count set
        rc = tdt_octree_geodesic_path(&ctx, &c.q, seeds.data(), n_seeds, regions, n_regions, goal, got.data(), n - 1, &n2, &cost2);
        ok = ok && rc == TDT_ERR_INVALID_VALUE && n2 == n;
      }
    }
  }
  ok = ok && want.size() >= c.min_reach && (size_t)passes >= c.min_passes;
  std::printf("%-22s depth %d medium %d w %d %d %d max %d mask %zu: |V| %zu reach %zu path %zu cost %ld passes %d field %d list %d %s\n", c.name,
              c.depth, c.q.medium, c.q.w[0], c.q.w[1], c.q.w[2], c.q.max_cost, n_regions, list.size(), want.size(), want_path.size(), want_cost,
              passes, (int)field_ok, (int)list_ok, ok ? "OK" : "MISMATCH");
  return ok ? 0 : 1;
}

static tdt_geodesic geo(int medium, int match, int w0, int w1, int w2, int max_cost, int material) {
  tdt_geodesic q{};
  q.medium = medium; q.match = match; q.w[0] = w0; q.w[1] = w1; q.w[2] = w2; q.max_cost = max_cost; q.material = material;
  return q;
}

int main() {
  int bad = 0;
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  std::mt19937 rng(11);
  auto random_grid = [&](int depth, unsigned per_mille) {
    Grid g(1 << depth);
    for (auto &m : g.m) if (rng() % 1000 < per_mille) m = 1 + (int)(rng() % 3);
    return g;
  };
  const int E = TDT_MEDIUM_EMPTY, S = TDT_MEDIUM_SOLID, BIG = 1 << 30;
  const std::vector<tdt_region> none;
  Grid g3 = random_grid(3, 650), g4 = random_grid(4, 600);
  g3.at(1, 1, 1) = 2; g3.at(6, 6, 5) = 0; g4.at(2, 3, 4) = 1; g4.at(12, 9, 3) = 0; g4.at(3, 3, 3) = 0;
  for (int x = 0; x < 16; x++) for (int y = 0; y < 16; y++) for (int z = 0; z < 16; z++)
    if (z < 2 || z > 5) g4.at(x, y, z) = 0;                // a slab: bbox(V), or a mask, keeps the domain to one layer of tiles
  bad += run(g3, {"random solid 6", 3, geo(S, -1, 1, 0, 0, BIG, -1), {{1, 1, 1}}, none, false, {6, 5, 5}, 20, 1, true});
  bad += run(g3, {"random empty 26 max 3", 3, geo(E, -1, 1, 1, 1, 3, 7), {{6, 6, 5}, {-1, 0, 0}}, none, false, {5, 5, 5}, 5, 1});
  bad += run(g3, {"max_cost 0", 3, geo(S, -1, 1, 1, 1, 0, -1), {{1, 1, 1}, {6, 6, 5}}, none, false, {1, 1, 1}, 1, 0});
  bad += run(g3, {"seeds off the medium", 3, geo(S, -1, 1, 1, 1, BIG, -1), {{6, 6, 5}, {9, 9, 9}}, none, false, {1, 1, 1}, 0, 0});
  bad += run(g3, {"no seeds", 3, geo(E, -1, 3, 4, 5, BIG, 0), {}, none, false, {1, 1, 1}, 0, 0});
  bad += run(g3, {"empty mask", 3, geo(S, -1, 1, 0, 0, BIG, -1), {{1, 1, 1}}, {tdt_region{TDT_SHAPE_BOX, {0, 0, 0}, {-1, -1, -1}, 0}}, true, {1, 1, 1}, 0, 0});
  bad += run(Grid(8), {"empty tree solid", 3, geo(S, -1, 1, 0, 0, BIG, -1), {{1, 1, 1}}, none, false, {1, 1, 1}, 0, 0});
  bad += run(Grid(8), {"empty tree empty 345", 3, geo(E, -1, 3, 4, 5, 9, 4), {{4, 4, 4}}, none, false, {6, 5, 4}, 20, 1});
  bad += run(g3, {"cheap diagonals 5 1 1", 3, geo(S, -1, 5, 1, 1, BIG, -1), {{1, 1, 1}}, none, false, {6, 5, 5}, 100, 1});
  bad += run(g3, {"no edges 7 0 2", 3, geo(E, -1, 7, 0, 2, 40, 2), {{6, 6, 5}}, none, false, {5, 5, 5}, 30, 1});
  bad += run(g4, {"chamfer one material", 4, geo(S, 0, 3, 4, 5, BIG, 9), {{2, 3, 4}}, none, false, {9, 9, 4}, 30, 1});
  {
    const std::vector<tdt_region> mask = {tdt_region{TDT_SHAPE_BOX, {1, 0, 2}, {9, 14, 5}, 0}, tdt_region{TDT_SHAPE_SPHERE, {11, 8, 4}, {2, 0, 0}, 0}};
    bad += run(g4, {"masked empty 2 3 0", 4, geo(E, -1, 2, 3, 0, 21, 1), {{12, 9, 3}, {3, 3, 3}}, mask, true, {5, 5, 5}, 50, 1, true});
  }
  {                                                        // a serpentine corridor in the plane z = 9 at depth 5: runs along y, so that
    Grid g(32);                                            // it re-enters the four tiles of its word again and again
    for (int i = 0; i < 14; i++) {
      for (int y = 1; y <= 30; y++) g.at(2 + 2 * i, y, 9) = 5;
      if (i < 13) g.at(3 + 2 * i, (i & 1) ? 1 : 30, 9) = 6;
    }
    bad += run(g, {"serpentine", 5, geo(S, -1, 1, 0, 0, BIG, -1), {{2, 1, 9}}, none, false, {28, 1, 9}, 400, 9});
    bad += run(g, {"serpentine cut", 5, geo(S, -1, 1, 0, 0, 200, 8), {{2, 1, 9}}, none, false, {28, 1, 9}, 201, 3});
  }
  {                                                        // across the word boundary of a row at depth 6, seeds at both ends
    Grid g(64);
    for (int x = 27; x <= 37; x++) g.at(x, 5, 40) = 3;
    g.at(32, 6, 41) = 4;
    bad += run(g, {"word boundary", 6, geo(S, -1, 1, 1, 1, BIG, -1), {{27, 5, 40}, {37, 5, 40}}, none, false, {32, 6, 41}, 12, 1});
  }
  std::printf(bad ? "FAILED %d\n" : "all ok\n", bad);
  return bad != 0;
}
