// voxel smoothing: drives the real entry points of tdt_smooth.hip on lists made here, against a brute force over every offset of
// the ball: the density, the support, the threshold test, the three modes, the mask, the iterations and the nearest voxel
#include <array>
#include "siblings.hpp"

// the pieces of the rebuild tail the unit's edit form calls: the list it hands to the builder is kept in g_edit
static uint32_t g_installed;
extern "C" const char *tdt_last_error(const tdt_ctx *c) { return c->err.c_str(); }
namespace tdt {
const std::vector<tdt_ctx *> &multi_members(tdt_ctx *) { static const std::vector<tdt_ctx *> none; return none; }
int build_cells_from_device(tdt_ctx *, const int32_t *d_vox, uint32_t n, int, tdt_buffer **out, uint32_t *n_cells) {
  g_edit.assign((const int4 *)d_vox, (const int4 *)d_vox + n);
  *out = nullptr; *n_cells = n + 1;
  return 0;
}
int install_cells(tdt_ctx *, tdt_ctx *, tdt_buffer *, uint32_t nc) { g_installed = nc; return 0; }
}

struct Off { int d2, dx, dy, dz; };
static std::vector<Off> ball(int r2) {
  std::vector<Off> b;
  int R = 0; while (R * R < r2) R++;
  for (int dx = -R; dx <= R; dx++) for (int dy = -R; dy <= R; dy++) for (int dz = -R; dz <= R; dz++)
    if (dx * dx + dy * dy + dz * dz <= r2) b.push_back(Off{dx * dx + dy * dy + dz * dz, dx, dy, dz});
  std::sort(b.begin(), b.end(), [](const Off &a, const Off &c) {
    return a.d2 != c.d2 ? a.d2 < c.d2 : a.dx != c.dx ? a.dx < c.dx : a.dy != c.dy ? a.dy < c.dy : a.dz < c.dz;
  });
  return b;
}
static void counts(const Grid &g, const std::vector<Off> &B, int x, int y, int z, int *d, int *n) {
  *d = 0; *n = 0;
  for (auto &o : B) {
    if (!g.in(x + o.dx, y + o.dy, z + o.dz)) continue;
    (*n)++;
    if (g.get(x + o.dx, y + o.dy, z + o.dz)) (*d)++;
  }
}
static Grid step(const Grid &g, const tdt_smooth &s, const std::vector<tdt_region> &mask) {
  const auto B = ball(s.radius2);
  Grid o(g.N);
  for (int x = 0; x < g.N; x++) for (int y = 0; y < g.N; y++) for (int z = 0; z < g.N; z++) {
    int d, n;
    counts(g, B, x, y, z, &d, &n);
    if (!s.border) n = (int)B.size();
    const bool t = s.threshold ? 65536ll * d >= (long long)s.threshold * n : 2 * d > n;
    const bool cur = g.get(x, y, z) != 0;
    bool keep = s.mode == TDT_SMOOTH_BOTH ? t : s.mode == TDT_SMOOTH_ADD ? (cur || t) : (cur && t);
    if (!mask.empty()) {
      bool in = false;
      for (auto &r : mask) in = in || region_has(r, x, y, z);
      if (!in) keep = cur;
    }
    if (!keep) continue;
    if (cur) { o.at(x, y, z) = g.get(x, y, z); continue; }
    if (s.material >= 0) { o.at(x, y, z) = s.material + 1; continue; }
    for (auto &f : B)
      if (g.in(x + f.dx, y + f.dy, z + f.dz) && g.get(x + f.dx, y + f.dy, z + f.dz)) { o.at(x, y, z) = g.get(x + f.dx, y + f.dy, z + f.dz); break; }
  }
  return o;
}

static int run_smooth(const char *name, int depth, const Grid &g, tdt_smooth s, const std::vector<tdt_region> &mask) {
  g_list = sorted_list(g); g_depth = depth;
  Grid want = g;
  for (int i = 0; i < s.iterations; i++) want = step(want, s, mask);
  tdt_ctx ctx{};
  std::vector<int4> gl;
  int rc = extract_list([&](int32_t *dst, size_t capacity, size_t *n) {
    return tdt_octree_extract_smooth(&ctx, &s, mask.data(), mask.size(), dst, capacity, n);
  }, gl);
  const auto wl = sorted_list(want);
  const bool ok = rc == 0 && same(gl, wl);
  // the edit form: the whole result goes to the builder, and the count it reports is the installed one
  uint32_t nc = 0;
  g_edit.clear(); g_installed = 0;
  rc = tdt_octree_smooth(&ctx, &s, mask.data(), mask.size(), &nc);
  const bool eok = rc == 0 && same(g_edit, wl) && nc == g_installed && nc == (wl.empty() ? 1u : (uint32_t)wl.size() + 1u);
  std::printf("%-10s depth %d r2 %3d it %2d thr %5d mode %d mat %3d border %d mask %zu: |V| %zu want %zu got %zu edit %zu %s\n", name, depth, s.radius2,
              s.iterations, s.threshold, s.mode, s.material, s.border, mask.size(), g_list.size(), wl.size(), gl.size(), g_edit.size(),
              ok && eok ? "OK" : "MISMATCH");
  return ok && eok ? 0 : 1;
}

static int run_field(const char *name, int depth, const Grid &g, std::array<int, 3> lo, std::array<int, 3> hi, int r2) {
  g_list = sorted_list(g); g_depth = depth;
  const auto B = ball(r2);
  tdt_ctx ctx{};
  size_t n = 0;
  int rc = tdt_octree_density_field(&ctx, lo.data(), hi.data(), r2, nullptr, nullptr, 0, &n);
  const int ex = hi[0] - lo[0] + 1, ey = hi[1] - lo[1] + 1, ez = hi[2] - lo[2] + 1;
  bool ok = rc == 0 && n == (size_t)ex * ey * ez && tdt_ball_size(r2) == (int)B.size();
  std::vector<int32_t> d(n + 1, 12345), s(n + 1, 12345), d2(n + 1, 12345);
  if (ok) ok = tdt_octree_density_field(&ctx, lo.data(), hi.data(), r2, d.data(), s.data(), n, &n) == 0;
  if (ok) ok = tdt_octree_density_field(&ctx, lo.data(), hi.data(), r2, d2.data(), nullptr, n, &n) == 0 && d == d2;
  size_t bad = d[n] != 12345 || s[n] != 12345;
  for (int z = lo[2]; ok && z <= hi[2]; z++) for (int y = lo[1]; y <= hi[1]; y++) for (int x = lo[0]; x <= hi[0]; x++) {
    const size_t at = ((size_t)(z - lo[2]) * ey + (y - lo[1])) * ex + (x - lo[0]);
    int wd, wn;
    counts(g, B, x, y, z, &wd, &wn);
    if (d[at] != wd || s[at] != wn) bad++;
  }
  std::printf("%-10s depth %d field r2 %3d box %d %d %d .. %d %d %d: |V| %zu bad %zu %s\n", name, depth, r2, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2],
              g_list.size(), bad, ok && !bad ? "OK" : "MISMATCH");
  return ok && !bad ? 0 : 1;
}

int main() {
  int bad = 0;
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  std::mt19937 rng(23);
  auto random_grid = [&](int depth, unsigned per_mille) {
    Grid g(1 << depth);
    for (auto &m : g.m) if (rng() % 1000 < per_mille) m = 1 + (int)(rng() % 254);
    return g;
  };
  const std::vector<tdt_region> mask = {tdt_region{TDT_SHAPE_BOX, {1, 0, 2}, {5, 9, 6}, 0}, tdt_region{TDT_SHAPE_SPHERE, {9, 9, 9}, {4, 0, 0}, 0}};
  {                                                        // a block is 256 real threads: every case costs seconds, so few of them
    const Grid half = random_grid(3, 500), dense = random_grid(3, 850), sparse = random_grid(3, 120);
    bad += run_smooth("half", 3, half, tdt_smooth{3, 1, 0, TDT_SMOOTH_BOTH, -1, 0}, {});
    bad += run_smooth("half", 3, half, tdt_smooth{2, 3, 0, TDT_SMOOTH_BOTH, -1, 1}, {});
    bad += run_smooth("half", 3, half, tdt_smooth{5, 2, 20000, TDT_SMOOTH_ADD, 7, 0}, mask);
    bad += run_smooth("dense", 3, dense, tdt_smooth{1, 1, 65536, TDT_SMOOTH_BOTH, -1, 1}, {});
    bad += run_smooth("dense", 3, dense, tdt_smooth{9, 2, 40000, TDT_SMOOTH_REMOVE, -1, 0}, {});
    bad += run_smooth("sparse", 3, sparse, tdt_smooth{4, 1, 1, TDT_SMOOTH_BOTH, -1, 0}, {});
    bad += run_smooth("sparse", 3, sparse, tdt_smooth{225, 1, 3000, TDT_SMOOTH_BOTH, -1, 1}, {});   // the ball is larger than the grid
    bad += run_field("half", 3, half, {0, 0, 0}, {7, 7, 7}, 6);
    bad += run_field("sparse", 3, sparse, {1, 0, 2}, {6, 7, 2}, 225);
  }
  {
    const Grid half = random_grid(4, 450);
    bad += run_smooth("half", 4, half, tdt_smooth{3, 2, 0, TDT_SMOOTH_BOTH, -1, 0}, mask);
    bad += run_smooth("half", 4, half, tdt_smooth{16, 1, 30000, TDT_SMOOTH_ADD, -1, 1}, {});
    bad += run_field("half", 4, half, {3, 1, 9}, {12, 15, 11}, 10);
  }
  {                                                        // a tied pair and a bar across the words of a row, at the tile's edge in y
    Grid g(64);
    g.at(31, 7, 40) = 3; g.at(33, 7, 40) = 9;
    for (int x = 29; x <= 35; x++) g.at(x, 8, 16) = 20 + x;
    bad += run_smooth("pairs", 6, g, tdt_smooth{4, 1, 1, TDT_SMOOTH_BOTH, -1, 0}, {});
    bad += run_field("pairs", 6, g, {28, 5, 39}, {36, 9, 41}, 225);
  }
  {
    Grid full(8);
    for (auto &m : full.m) m = 2;
    bad += run_smooth("full", 3, full, tdt_smooth{3, 2, 0, TDT_SMOOTH_BOTH, -1, 0}, {});
    bad += run_smooth("full", 3, full, tdt_smooth{3, 2, 0, TDT_SMOOTH_BOTH, -1, 1}, {});
    bad += run_smooth("empty", 3, Grid(8), tdt_smooth{4, 1, 0, TDT_SMOOTH_BOTH, -1, 0}, {});
    bad += run_field("empty", 3, Grid(8), {0, 1, 2}, {7, 1, 5}, 16);
    Grid one(8); one.at(3, 4, 5) = 8;
    bad += run_smooth("one", 3, one, tdt_smooth{2, 1, 0, TDT_SMOOTH_BOTH, -1, 0}, {});       // a single voxel vanishes under majority
  }
  std::printf(bad ? "FAILED %d\n" : "all ok\n", bad);
  return bad != 0;
}
