// exact distance: drives the real entry points of tdt_distance.hip on lists made here, against an all-pairs brute force and
// the ops' definitions
#include <array>
#include "siblings.hpp"

// the set voxels, in lexicographic (x, y, z) order
static std::vector<std::array<int, 3>> points(const Grid &g) {
  std::vector<std::array<int, 3>> p;
  for (int x = 0; x < g.N; x++) for (int y = 0; y < g.N; y++) for (int z = 0; z < g.N; z++) if (g.get(x, y, z)) p.push_back({x, y, z});
  return p;
}
// all pairs: the squared distance to the nearest set voxel and that voxel (the first at the minimum in lexicographic order)
static long nearest(const std::vector<std::array<int, 3>> &P, int x, int y, int z, std::array<int, 3> *who) {
  long best = -1;
  for (auto &p : P) {
    const long d = (long)(p[0] - x) * (p[0] - x) + (long)(p[1] - y) * (p[1] - y) + (long)(p[2] - z) * (p[2] - z);
    if (best < 0 || d < best) { best = d; if (who) *who = p; }
  }
  return best;
}
static Grid dilate(const Grid &g, int r2, int material) {
  Grid o = g;
  const auto P = points(g);
  if (P.empty()) return o;
  for (int x = 0; x < g.N; x++) for (int y = 0; y < g.N; y++) for (int z = 0; z < g.N; z++) {
    if (g.get(x, y, z)) continue;
    std::array<int, 3> w;
    if (nearest(P, x, y, z, &w) <= r2) o.at(x, y, z) = material >= 0 ? material + 1 : g.get(w[0], w[1], w[2]);
  }
  return o;
}
// by the definition: every lattice point of the ball is set, or outside the grid with border 1
static Grid erode(const Grid &g, int r2, int border) {
  Grid o = g;
  int R = 0; while ((R + 1) * (R + 1) <= r2) R++;
  for (int x = 0; x < g.N; x++) for (int y = 0; y < g.N; y++) for (int z = 0; z < g.N; z++) {
    if (!g.get(x, y, z)) continue;
    bool keep = true;
    for (int dx = -R; dx <= R && keep; dx++) for (int dy = -R; dy <= R && keep; dy++) for (int dz = -R; dz <= R && keep; dz++) {
      if (dx * dx + dy * dy + dz * dz > r2) continue;
      if (g.in(x + dx, y + dy, z + dz)) keep = g.get(x + dx, y + dy, z + dz) != 0; else keep = border == 1;
    }
    if (!keep) o.at(x, y, z) = 0;
  }
  return o;
}
static Grid apply(const Grid &g, int op, int r2, int material, int border) {
  switch (op) {
    case TDT_MORPH_DILATE: return dilate(g, r2, material);
    case TDT_MORPH_ERODE: return erode(g, r2, border);
    case TDT_MORPH_OPEN: {                                 // a subset of V: the original materials
      Grid o = dilate(erode(g, r2, 1), r2, material);
      for (size_t i = 0; i < o.m.size(); i++) if (o.m[i]) o.m[i] = g.m[i];
      return o;
    }
    case TDT_MORPH_CLOSE: return erode(dilate(g, r2, material), r2, 1);
    default: { Grid e = erode(g, r2, border), o = g; for (size_t i = 0; i < o.m.size(); i++) if (e.m[i]) o.m[i] = 0; return o; }
  }
}

static int run_round(const char *name, int depth, const Grid &g, int op, int r2, int material, int border, const std::vector<tdt_region> &mask) {
  g_list = sorted_list(g); g_depth = depth;
  Grid want = apply(g, op, r2, material, border);
  if (!mask.empty())
    for (int x = 0; x < g.N; x++) for (int y = 0; y < g.N; y++) for (int z = 0; z < g.N; z++) {
      bool in = false;
      for (auto &r : mask) in = in || region_has(r, x, y, z);
      if (!in) want.at(x, y, z) = g.get(x, y, z);
    }
  tdt_ctx ctx{};
  tdt_round q{op, r2, material, border};
  std::vector<int4> gl;
  int rc = extract_list([&](int32_t *dst, size_t capacity, size_t *n) {
    return tdt_octree_extract_morph_round(&ctx, &q, mask.data(), mask.size(), dst, capacity, n);
  }, gl);
  const size_t n = gl.size();
  const auto wl = sorted_list(want);
  bool ok = rc == 0 && same(gl, wl);
  // the edit form's delta: exactly the voxels that differ, new ones with their material, for the right op
  uint32_t nc = 0;
  rc = tdt_octree_morph_round(&ctx, &q, mask.data(), mask.size(), &nc);
  const bool grows = op == TDT_MORPH_DILATE || op == TDT_MORPH_CLOSE;
  Grid diff(g.N);
  for (size_t i = 0; i < diff.m.size(); i++) if ((g.m[i] != 0) != (want.m[i] != 0)) diff.m[i] = grows ? want.m[i] : g.m[i];
  const std::vector<int4> dl = morton_sorted(g_edit);
  const bool dok = rc == 0 && g_edit_op == (grows ? TDT_REGION_FILL : TDT_REGION_CLEAR) && same(dl, sorted_list(diff));
  std::printf("%-22s depth %d op %d r2 %4d mat %3d border %d mask %zu: |V| %zu want %zu got %zu delta %zu %s\n", name, depth, op, r2, material,
              border, mask.size(), g_list.size(), wl.size(), n, dl.size(), ok && dok ? "OK" : "MISMATCH");
  return ok && dok ? 0 : 1;
}

static int run_field(const char *name, int depth, const Grid &g, std::array<int, 3> lo, std::array<int, 3> hi, int max_d2, int border) {
  g_list = sorted_list(g); g_depth = depth;
  const auto P = points(g);
  Grid c(g.N);
  for (size_t i = 0; i < c.m.size(); i++) c.m[i] = !g.m[i];
  const auto C = points(c);
  tdt_ctx ctx{};
  size_t n = 0;
  int rc = tdt_octree_distance_field(&ctx, lo.data(), hi.data(), max_d2, border, nullptr, nullptr, 0, &n);
  const int ex = hi[0] - lo[0] + 1, ey = hi[1] - lo[1] + 1, ez = hi[2] - lo[2] + 1;
  bool ok = rc == 0 && n == (size_t)ex * ey * ez;
  std::vector<int32_t> f(n + 1, 12345), nr(3 * n + 3, 12345);
  if (ok) ok = tdt_octree_distance_field(&ctx, lo.data(), hi.data(), max_d2, border, f.data(), nr.data(), n, &n) == 0;
  size_t bad = 0;
  for (int z = lo[2]; ok && z <= hi[2]; z++) for (int y = lo[1]; y <= hi[1]; y++) for (int x = lo[0]; x <= hi[0]; x++) {
    const size_t at = ((size_t)(z - lo[2]) * ey + (y - lo[1])) * ex + (x - lo[0]);
    int want, w[3] = {-1, -1, -1};
    if (g.get(x, y, z)) {
      long d = C.empty() ? -1 : nearest(C, x, y, z, nullptr);
      if (!border) {
        long e = std::min({x + 1, y + 1, z + 1, g.N - x, g.N - y, g.N - z});
        d = d < 0 || e * e < d ? e * e : d;
      }
      want = -(int)(d < 0 || d > max_d2 ? max_d2 + 1 : d);
      w[0] = x; w[1] = y; w[2] = z;
    } else {
      std::array<int, 3> who{};
      const long d = P.empty() ? -1 : nearest(P, x, y, z, &who);
      want = (int)(d < 0 || d > max_d2 ? max_d2 + 1 : d);
      if (d >= 0 && d <= max_d2) { w[0] = who[0]; w[1] = who[1]; w[2] = who[2]; }
    }
    if (f[at] != want || nr[3 * at] != w[0] || nr[3 * at + 1] != w[1] || nr[3 * at + 2] != w[2]) bad++;
  }
  std::printf("%-22s depth %d field max_d2 %4d border %d box %d %d %d .. %d %d %d: |V| %zu bad %zu %s\n", name, depth, max_d2, border, lo[0], lo[1],
              lo[2], hi[0], hi[1], hi[2], g_list.size(), bad, ok && !bad ? "OK" : "MISMATCH");
  return ok && !bad ? 0 : 1;
}

int main() {
  int bad = 0;
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  std::mt19937 rng(11);
  auto random_grid = [&](int depth, unsigned per_mille) {
    Grid g(1 << depth);
    for (auto &m : g.m) if (rng() % 1000 < per_mille) m = 1 + (int)(rng() % 254);
    return g;
  };
  const std::vector<tdt_region> mask = {tdt_region{TDT_SHAPE_BOX, {1, 0, 2}, {5, 9, 6}, 0}, tdt_region{TDT_SHAPE_SPHERE, {9, 9, 9}, {4, 0, 0}, 0}};
  {                                                        // a block is 256 real threads: every case costs seconds, so few of them
    const Grid sparse = random_grid(3, 60), dense = random_grid(3, 850);
    bad += run_round("sparse", 3, sparse, TDT_MORPH_DILATE, 2, -1, 0, {});
    bad += run_round("sparse", 3, sparse, TDT_MORPH_CLOSE, 3, -1, 0, {});
    bad += run_round("sparse", 3, sparse, TDT_MORPH_CLOSE, 5, 7, 0, mask);
    bad += run_round("dense", 3, dense, TDT_MORPH_ERODE, 1, -1, 0, {});
    bad += run_round("dense", 3, dense, TDT_MORPH_SHELL, 3, -1, 1, mask);
    bad += run_round("dense", 3, dense, TDT_MORPH_OPEN, 2, -1, 0, {});
    bad += run_field("sparse", 3, sparse, {0, 0, 0}, {7, 7, 7}, 9, 0);
    bad += run_field("dense", 3, dense, {1, 0, 2}, {6, 7, 2}, 4096, 1);
  }
  {
    const Grid sparse = random_grid(4, 40), dense = random_grid(4, 900);
    bad += run_round("sparse", 4, sparse, TDT_MORPH_DILATE, 16, 200, 0, mask);
    bad += run_round("dense", 4, dense, TDT_MORPH_ERODE, 5, -1, 0, {});
    bad += run_field("dense", 4, dense, {1, 0, 2}, {12, 15, 5}, 1, 0);
  }
  {                                                        // pairs across the words of a row: an axis tie at x = 32, a diagonal tie
    Grid g(64);
    g.at(31, 5, 40) = 3; g.at(33, 5, 40) = 9;
    g.at(30, 7, 41) = 6; g.at(31, 6, 41) = 7;
    bad += run_round("pairs", 6, g, TDT_MORPH_DILATE, 9, -1, 0, {});
    bad += run_round("pairs", 6, g, TDT_MORPH_CLOSE, 5, -1, 0, {});
    bad += run_field("pairs", 6, g, {28, 3, 39}, {36, 8, 42}, 4, 0);
  }
  {
    Grid full(8);
    for (auto &m : full.m) m = 2;
    bad += run_round("full", 3, full, TDT_MORPH_ERODE, 5, -1, 0, {});
    bad += run_round("full", 3, full, TDT_MORPH_SHELL, 4, -1, 1, {});
    bad += run_field("full", 3, full, {0, 0, 0}, {7, 7, 7}, 16, 0);
    bad += run_round("empty", 3, Grid(8), TDT_MORPH_DILATE, 4, -1, 0, {});
    bad += run_field("empty", 3, Grid(8), {0, 1, 2}, {7, 1, 5}, 16, 0);
    Grid one(2); one.at(1, 0, 1) = 8;
    bad += run_round("depth 1", 1, one, TDT_MORPH_DILATE, 4096, -1, 0, {});
    bad += run_round("depth 1", 1, one, TDT_MORPH_ERODE, 1, -1, 1, {});
  }
  std::printf(bad ? "FAILED %d\n" : "all ok\n", bad);
  return bad != 0;
}
