// affine transforms: drives the real entry points of tdt_xform.hip on lists made here, against a brute force over every
// destination voxel
#include "siblings.hpp"
// floor(v / 2^17) by a division and a correction, where the unit shifts
static __int128 floor17(__int128 v) { __int128 q = v / 131072; if (v % 131072 < 0) q--; return q; }

static tdt_xform make(std::initializer_list<long> a, std::initializer_list<long long> t) {
  tdt_xform x{};
  int i = 0; for (long v : a) x.a[i++] = (int32_t)v;
  i = 0; for (long long v : t) x.t[i++] = v;
  x.material = -1;
  for (int k = 0; k < 3; k++) x.dst_hi[k] = INT32_MAX;
  return x;
}

// min_results: the case must not be vacuous
static int run(const char *name, int depth, const Grid &g, tdt_xform x, const std::vector<tdt_region> &mask, bool masked, size_t min_results) {
  g_list = sorted_list(g); g_depth = depth;
  Grid want(g.N);
  for (int px = 0; px < g.N; px++) for (int py = 0; py < g.N; py++) for (int pz = 0; pz < g.N; pz++) {
    const int p[3] = {px, py, pz};
    bool in = true;
    __int128 s[3];
    for (int i = 0; i < 3; i++) {
      in = in && p[i] >= x.dst_lo[i] && p[i] <= x.dst_hi[i];
      __int128 v = x.t[i];
      for (int j = 0; j < 3; j++) v += (__int128)x.a[3 * i + j] * (2 * p[j] + 1);
      s[i] = floor17(v);
      in = in && s[i] >= 0 && s[i] < g.N;
    }
    if (!in) continue;
    const int m = g.get((int)s[0], (int)s[1], (int)s[2]);
    if (!m) continue;
    bool sel = !masked;
    for (auto &r : mask) sel = sel || region_has(r, (long)s[0], (long)s[1], (long)s[2]);
    if (sel) want.at(px, py, pz) = x.material >= 0 ? x.material + 1 : m;
  }
  const auto wl = sorted_list(want);
  tdt_ctx ctx{};
  const tdt_region *regions = masked ? mask.data() : nullptr;
  const size_t n_regions = masked ? mask.size() : 0;
  std::vector<int4> gl;
  int rc = extract_list([&](int32_t *dst, size_t capacity, size_t *n) {
    return tdt_octree_extract_transform(&ctx, &x, regions, n_regions, dst, capacity, n);
  }, gl);
  const size_t n = gl.size();
  uint32_t bricks[2] = {0, 0};
  tdt_debug_xform_bricks(&ctx, bricks);
  bool ok = rc == 0 && same(gl, wl) && wl.size() >= min_results && bricks[1] <= bricks[0];
  uint32_t nc = 0;
  rc = tdt_octree_transform(&ctx, &x, TDT_REGION_FILL, regions, n_regions, &nc);
  ok = ok && rc == 0 && g_edit_op == TDT_REGION_FILL && same(g_edit, wl);
  std::printf("%-18s depth %d mask %zu: |V| %zu want %zu got %zu bricks %u kept %u %s\n", name, depth, n_regions, g_list.size(), wl.size(), n,
              bricks[0], bricks[1], ok ? "OK" : "MISMATCH");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  std::mt19937 rng(5);
  auto random_grid = [&](int depth, unsigned per_mille) {
    Grid g(1 << depth);
    for (auto &m : g.m) if (rng() % 1000 < per_mille) m = 1 + (int)(rng() % 254);
    return g;
  };
  const long U = 65536;
  const std::vector<tdt_region> none;
  const Grid g3 = random_grid(3, 300), g4 = random_grid(4, 250), g5 = random_grid(5, 30);
  bad += run("identity", 3, g3, make({U, 0, 0, 0, U, 0, 0, 0, U}, {0, 0, 0}), none, false, 100);
  bad += run("move 1 -3 5", 4, g4, make({U, 0, 0, 0, U, 0, 0, 0, U}, {-131072, 3 * 131072, -5 * 131072}), none, false, 100);
  bad += run("move -N+1", 4, g4, make({U, 0, 0, 0, U, 0, 0, 0, U}, {15 * 131072, 0, 0}), none, false, 10);
  {                                                        // turns: a = 65536 R^-1, t = 65536 (P - R^-1 P)
    const std::vector<tdt_region> mask = {tdt_region{TDT_SHAPE_BOX, {1, 0, 2}, {8, 14, 15}, 0}, tdt_region{TDT_SHAPE_SPHERE, {8, 8, 5}, {5, 0, 0}, 0}};
    bad += run("turn z even", 4, g4, make({0, U, 0, -U, 0, 0, 0, 0, U}, {0, 32 * U, 0}), mask, true, 100);
    // about x, three turns = the inverse of one: y' = z, z' = -y; pivot2 (., 7, 9): equal parity
    bad += run("turn x odd", 3, g3, make({U, 0, 0, 0, 0, -U, 0, U, 0}, {0, (7 + 9) * U, (9 - 7) * U}), none, false, 50);
    // unequal parity: centres land on faces, the floor picks a side
    bad += run("turn z uneven", 3, g3, make({0, U, 0, -U, 0, 0, 0, 0, U}, {(8 - 7) * U, (7 + 8) * U, 0}), none, false, 50);
  }
  {
    tdt_xform x = make({U, 0, 0, 0, -U, 0, 0, 0, U}, {0, 2 * 16 * U, 0});
    x.material = 41;
    bad += run("mirror y fixed", 4, g4, x, none, false, 100);
  }
  bad += run("x2", 4, g4, make({U / 2, 0, 0, 0, U / 2, 0, 0, 0, U / 2}, {0, 0, 0}), none, false, 500);
  bad += run("x1/2", 5, g5, make({2 * U, 0, 0, 0, 2 * U, 0, 0, 0, 2 * U}, {0, 0, 0}), none, false, 20);
  {
    tdt_xform x = make({43691, 0, 0, 0, 43691, 0, 0, 0, 43691}, {(U - 43691) * 5, (U - 43691) * 6, (U - 43691) * 7});
    for (int k = 0; k < 3; k++) { x.dst_lo[k] = 3; x.dst_hi[k] = 12; }
    bad += run("x3/2 dst 3..12", 4, g4, x, none, false, 100);
  }
  {                                                        // 30 degrees about z through (6.5, 8.25, .): rint(65536 R^-1)
    const std::vector<tdt_region> mask = {tdt_region{TDT_SHAPE_BOX, {1, 0, 2}, {8, 14, 15}, 0}, tdt_region{TDT_SHAPE_SPHERE, {8, 8, 5}, {5, 0, 0}, 0}};
    bad += run("rotate 30", 4, g4, make({56756, 32768, 0, -32768, 56756, 0, 0, 0, U}, {-426530, 570857, 0}), mask, true, 100);
    bad += run("empty mask", 4, g4, make({U, 0, 0, 0, U, 0, 0, 0, U}, {0, 0, 0}), {tdt_region{TDT_SHAPE_BOX, {0, 0, 0}, {-1, -1, -1}, 0}}, true, 0);
  }
  {                                                        // entries of +-2^20; an offset of 2^40 leaves the grid
    Grid g(8);
    g.at(0, 0, 0) = 3; g.at(7, 7, 7) = 9; g.at(3, 4, 1) = 77;
    const long A = 1l << 20;
    bad += run("2^20 entries", 3, g, make({A, -A, 0, 0, A, -A, A, 0, A}, {3 * 131072, 4 * 131072, (1 - 48) * 131072}), none, false, 1);   // p = (1, 1, 1) -> (3, 4, 1)
    bad += run("2^20 row", 3, g, make({A, A, A, 0, U, 0, 0, 0, U}, {-24 * 131072, 0, 0}), none, false, 1);             // p = 0 -> 0
    bad += run("t 2^40", 3, g, make({U, 0, 0, 0, U, 0, 0, 0, U}, {1ll << 40, -(1ll << 40), 0}), none, false, 0);
    bad += run("empty tree", 3, Grid(8), make({U, 0, 0, 0, U, 0, 0, 0, U}, {0, 0, 0}), none, false, 0);
  }
  {                                                        // across the word boundary of a row
    Grid g(64);
    g.at(31, 5, 40) = 3; g.at(32, 5, 40) = 9; g.at(33, 6, 41) = 6;
    bad += run("word boundary", 6, g, make({U, 0, 0, 0, U, 0, 0, 0, U}, {131072, 0, -131072}), none, false, 3);
  }
  std::printf(bad ? "FAILED %d\n" : "all ok\n", bad);
  return bad != 0;
}
