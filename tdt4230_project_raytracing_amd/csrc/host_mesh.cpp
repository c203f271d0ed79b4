// Host side of triangle-mesh voxelisation (include/tdt_host.h "triangle meshes"): float vertices -> the fixed-point vertices
// tdt_voxelize_triangles takes (tdt_mesh_quantize, tdt_mesh_fit), and a minimal ASCII PLY mesh reader.  The reader is its
// own grammar, not tdt_ply_parse's: that one restates the reference's point loader with its quirks.  And the way back: the
// quads of tdt_octree_extract_surface -> a welded indexed mesh (tdt_quads_to_mesh), and that mesh as ASCII PLY (tdt_ply_mesh_write).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "tdt_host.h"

extern "C" void tdt_host_set_error(const char *msg);   // host_scene.cpp

struct tdt_ply_mesh {
  std::vector<float> xyz;
  std::vector<uint32_t> tri;
  int64_t faces = 0;
};

namespace {

constexpr int kInvalidValue = 0x0501;
constexpr double kUnit = 64.0;                // 2^TDT_MESH_FRAC
constexpr double kCoordMax = 262144.0;        // TDT_MESH_COORD_MAX

int fail(const std::string &m) { tdt_host_set_error(m.c_str()); return kInvalidValue; }

// whitespace-separated words of one buffer, line-aware: the header is read by lines, the body by words
struct Reader {
  const char *p, *end;
  size_t line = 1;
  bool next_line(std::string &out) {           // without its LF / CRLF
    if (p >= end) return false;
    const char *e = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
    const char *stop = e ? e : end;
    out.assign(p, stop);
    if (!out.empty() && out.back() == '\r') out.pop_back();
    p = e ? e + 1 : end;
    line++;
    return true;
  }
  bool next_word(std::string &out) {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) { if (*p == '\n') line++; p++; }
    if (p >= end) return false;
    const char *s = p;
    while (p < end && !(*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) p++;
    out.assign(s, p);
    return true;
  }
};

std::vector<std::string> split(const std::string &s) {
  std::vector<std::string> w;
  size_t i = 0;
  while (i < s.size()) {
    while (i < s.size() && (s[i] == ' ' || s[i] == '\t')) i++;
    size_t j = i;
    while (j < s.size() && s[j] != ' ' && s[j] != '\t') j++;
    if (j > i) w.push_back(s.substr(i, j - i));
    i = j;
  }
  return w;
}

bool to_double(const std::string &w, double &v) {
  char *e = nullptr;
  v = std::strtod(w.c_str(), &e);
  return !w.empty() && e == w.c_str() + w.size() && std::isfinite(v);
}
bool to_index(const std::string &w, int64_t &v) {
  char *e = nullptr;
  v = std::strtoll(w.c_str(), &e, 10);
  return !w.empty() && e == w.c_str() + w.size();
}

bool is_scalar_type(const std::string &t) {
  static const char *k[] = {"char", "uchar", "short", "ushort", "int", "uint", "float", "double", "int8", "uint8", "int16", "uint16",
                            "int32", "uint32", "float32", "float64"};
  for (const char *n : k) if (t == n) return true;
  return false;
}

int parse(const char *data, size_t bytes, tdt_ply_mesh &M) {
  Reader R{data, data + bytes};
  std::string ln;
  auto at = [&R]() { return " (line " + std::to_string(R.line - 1) + ")"; };
  if (!R.next_line(ln) || ln != "ply") return fail("not a PLY file: the first line must be 'ply'");
  if (!R.next_line(ln) || split(ln) != std::vector<std::string>{"format", "ascii", "1.0"})
    return fail("only 'format ascii 1.0' is read, not '" + ln + "'");
  int64_t nv = -1, nf = -1;
  int element = 0;                             // 1 vertex, 2 face
  int vertex_props = 0, face_props = 0;
  bool ended = false;
  while (R.next_line(ln)) {
    const std::vector<std::string> w = split(ln);
    if (w.empty() || w[0] == "comment" || w[0] == "obj_info") continue;
    if (w[0] == "end_header") { ended = true; break; }
    if (w[0] == "element") {
      int64_t n = 0;
      if (w.size() != 3 || !to_index(w[2], n) || n < 0 || n > (int64_t{1} << 31)) return fail("bad element line '" + ln + "'" + at());
      if (w[1] == "vertex" && nv < 0 && nf < 0) { nv = n; element = 1; }
      else if (w[1] == "face" && nv >= 0 && nf < 0) { nf = n; element = 2; }
      else return fail("elements must be 'vertex' then 'face', not '" + ln + "'" + at());
    } else if (w[0] == "property") {
      if (element == 1) {
        if (w.size() != 3 || !is_scalar_type(w[1])) return fail("bad vertex property '" + ln + "'" + at());
        static const char *xyz[3] = {"x", "y", "z"};
        if (vertex_props < 3 && (w[2] != xyz[vertex_props] || (w[1] != "float" && w[1] != "double" && w[1] != "float32" && w[1] != "float64")))
          return fail("the first three vertex properties must be float or double x, y, z, not '" + ln + "'" + at());
        vertex_props++;
      } else if (element == 2) {
        const bool count_ok = w.size() == 5 && (w[2] == "uchar" || w[2] == "uint8");
        const bool index_ok = w.size() == 5 && (w[3] == "int" || w[3] == "uint" || w[3] == "int32" || w[3] == "uint32");
        if (w.size() != 5 || w[1] != "list" || !count_ok || !index_ok || (w[4] != "vertex_indices" && w[4] != "vertex_index") || face_props)
          return fail("the face element takes one 'property list uchar int vertex_indices', not '" + ln + "'" + at());
        face_props++;
      } else {
        return fail("a property before any element" + at());
      }
    } else {
      return fail("unknown header line '" + ln + "'" + at());
    }
  }
  if (!ended) return fail("the header has no end_header");
  if (nv < 0 || vertex_props < 3) return fail("the header declares no vertex element with x, y, z");
  if (nf < 0 || face_props != 1) return fail("the header declares no face element with a vertex_indices list");
  std::string w;
  M.xyz.reserve(static_cast<size_t>(3 * nv));
  for (int64_t i = 0; i < nv; i++)
    for (int k = 0; k < vertex_props; k++) {
      double v = 0;
      if (!R.next_word(w)) return fail("truncated data: vertex " + std::to_string(i) + " of " + std::to_string(nv));
      if (!to_double(w, v)) return fail("vertex " + std::to_string(i) + ": '" + w + "' is not a finite number");
      if (k < 3) M.xyz.push_back(static_cast<float>(v));
    }
  std::vector<uint32_t> poly;
  for (int64_t f = 0; f < nf; f++) {
    int64_t k = 0;
    if (!R.next_word(w)) return fail("truncated data: face " + std::to_string(f) + " of " + std::to_string(nf));
    if (!to_index(w, k) || k < 0 || k > 255) return fail("face " + std::to_string(f) + ": bad index count '" + w + "'");
    if (k < 3) return fail("face " + std::to_string(f) + ": " + std::to_string(k) + " indices (a polygon needs at least 3)");
    poly.clear();
    for (int64_t j = 0; j < k; j++) {
      int64_t v = 0;
      if (!R.next_word(w)) return fail("truncated data: face " + std::to_string(f) + " of " + std::to_string(nf));
      if (!to_index(w, v)) return fail("face " + std::to_string(f) + ": '" + w + "' is not an index");
      if (v < 0 || v >= nv) return fail("face " + std::to_string(f) + ": vertex index " + std::to_string(v) + " >= " + std::to_string(nv) + " vertices");
      poly.push_back(static_cast<uint32_t>(v));
    }
    for (size_t j = 1; j + 1 < poly.size(); j++) { M.tri.push_back(poly[0]); M.tri.push_back(poly[j]); M.tri.push_back(poly[j + 1]); }
  }
  if (R.next_word(w)) return fail("data after the last face: '" + w + "'");
  M.faces = nf;
  return 0;
}

}  // namespace

extern "C" {

int tdt_mesh_quantize(const float *xyz, size_t n, double scale, const double offset[3], int32_t *out) {
  if ((n && (!xyz || !out)) || !offset) return fail("null argument");
  if (!std::isfinite(scale) || !std::isfinite(offset[0]) || !std::isfinite(offset[1]) || !std::isfinite(offset[2]))
    return fail("scale and offset must be finite");
  for (size_t i = 0; i < 3 * n; i++) {                       // the check first: nothing is written on an error
    const double v = (static_cast<double>(xyz[i]) * scale + offset[i % 3]) * kUnit;
    if (!(std::fabs(v) <= kCoordMax + 0.5) || std::fabs(std::nearbyint(v)) > kCoordMax)
      return fail("vertex " + std::to_string(i / 3) + ": coordinate " + std::to_string(v / kUnit) + " voxels is not finite or beyond +-4096");
  }
  for (size_t i = 0; i < 3 * n; i++)
    out[i] = static_cast<int32_t>(std::llrint((static_cast<double>(xyz[i]) * scale + offset[i % 3]) * kUnit));
  return 0;
}

int tdt_mesh_fit(const float *xyz, size_t n, const int32_t lo[3], const int32_t hi[3], double *scale, double offset[3]) {
  if (!xyz || !lo || !hi || !scale || !offset) return fail("null argument");
  if (n == 0) return fail("an empty mesh cannot be fitted");
  double mn[3], mx[3];
  for (int a = 0; a < 3; a++) {
    if (hi[a] < lo[a]) return fail("the box is empty");
    mn[a] = mx[a] = static_cast<double>(xyz[a]);
  }
  for (size_t i = 0; i < 3 * n; i++) {
    const double v = static_cast<double>(xyz[i]);
    if (!std::isfinite(v)) return fail("vertex " + std::to_string(i / 3) + " is not finite");
    mn[i % 3] = v < mn[i % 3] ? v : mn[i % 3];
    mx[i % 3] = v > mx[i % 3] ? v : mx[i % 3];
  }
  double s = 1.0;
  bool any = false;
  for (int a = 0; a < 3; a++) {
    const double ext = mx[a] - mn[a], room = (static_cast<double>(hi[a]) + 1.0) - static_cast<double>(lo[a]);
    if (ext > 0) { const double r = room / ext; s = (!any || r < s) ? r : s; any = true; }
  }
  *scale = s;
  for (int a = 0; a < 3; a++)
    offset[a] = (static_cast<double>(lo[a]) + (static_cast<double>(hi[a]) + 1.0)) * 0.5 - (mn[a] + mx[a]) * 0.5 * s;
  return 0;
}

int tdt_ply_mesh_parse(const void *data, size_t bytes, tdt_ply_mesh **out) {
  if (!data || !out) return fail("null argument");
  *out = nullptr;
  tdt_ply_mesh *m = new (std::nothrow) tdt_ply_mesh;
  if (!m) return fail("out of memory");
  int rc;
  try {
    rc = parse(static_cast<const char *>(data), bytes, *m);
  } catch (const std::bad_alloc &) { rc = fail("out of memory"); }
  if (rc) { delete m; return rc; }
  *out = m;
  return 0;
}

void tdt_ply_mesh_destroy(tdt_ply_mesh *m) { delete m; }

int tdt_ply_mesh_info(const tdt_ply_mesh *m, int64_t *n_vertices, int64_t *n_faces, int64_t *n_triangles) {
  if (!m) return fail("null argument");
  if (n_vertices) *n_vertices = static_cast<int64_t>(m->xyz.size() / 3);
  if (n_faces) *n_faces = m->faces;
  if (n_triangles) *n_triangles = static_cast<int64_t>(m->tri.size() / 3);
  return 0;
}

const float *tdt_ply_mesh_vertices(const tdt_ply_mesh *m) { return m && !m->xyz.empty() ? m->xyz.data() : nullptr; }
const uint32_t *tdt_ply_mesh_triangles(const tdt_ply_mesh *m) { return m && !m->tri.empty() ? m->tri.data() : nullptr; }

int tdt_quads_to_mesh(const int32_t *quads, size_t n_quads, int32_t *vertices, size_t vertex_capacity, size_t *n_vertices,
                      uint32_t *triangles, int32_t *materials, size_t triangle_capacity, size_t *n_triangles) {
  if (!n_vertices || !n_triangles || (n_quads && !quads)) return fail("null argument");
  *n_vertices = *n_triangles = 0;
  if (n_quads > (size_t{1} << 30)) return fail("more than 2^30 quads");
  constexpr int64_t kMaxVoxel = static_cast<int64_t>(kCoordMax / kUnit);
  try {
    // the four emitted corners of every quad as x << 42 | y << 21 | z (units <= 2^18): ascending keys = ascending (x, y, z)
    std::vector<uint64_t> corner(4 * n_quads);
    for (size_t q = 0; q < n_quads; q++) {
      const int32_t *Q = quads + 8 * q;
      const int f = Q[0];
      if (f < 0 || f > 5) return fail("quad " + std::to_string(q) + ": face " + std::to_string(f) + " is not 0..5");
      if (Q[5] < 1 || Q[6] < 1) return fail("quad " + std::to_string(q) + ": a size below 1");
      const int a = f >> 1, u = (a + 1) % 3, v = (a + 2) % 3;
      int64_t c[4][3];
      for (int k = 0; k < 4; k++) for (int d = 0; d < 3; d++) c[k][d] = Q[2 + d];
      c[1][u] += Q[5]; c[2][u] += Q[5]; c[2][v] += Q[6]; c[3][v] += Q[6];
      for (int d = 0; d < 3; d++)
        if (c[0][d] < 0 || c[2][d] > kMaxVoxel) return fail("quad " + std::to_string(q) + ": a corner outside 0..4096 voxels");
      static const int order[2][4] = {{0, 3, 2, 1}, {0, 1, 2, 3}};
      for (int k = 0; k < 4; k++) {
        const int64_t *p = c[order[f & 1][k]];
        corner[4 * q + k] = static_cast<uint64_t>(p[0] * 64) << 42 | static_cast<uint64_t>(p[1] * 64) << 21 | static_cast<uint64_t>(p[2] * 64);
      }
    }
    std::vector<uint64_t> uniq(corner);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    *n_vertices = uniq.size();
    *n_triangles = 2 * n_quads;
    if (!vertices && !triangles && !materials) return 0;
    if ((!vertices && *n_vertices) || (!triangles && *n_triangles)) return fail("vertices and triangles are both required to fill");
    if (vertex_capacity < *n_vertices) return fail("capacity " + std::to_string(vertex_capacity) + " < " + std::to_string(*n_vertices) + " vertices");
    if (triangle_capacity < *n_triangles)
      return fail("capacity " + std::to_string(triangle_capacity) + " < " + std::to_string(*n_triangles) + " triangles");
    for (size_t i = 0; i < uniq.size(); i++) {
      vertices[3 * i] = static_cast<int32_t>(uniq[i] >> 42);
      vertices[3 * i + 1] = static_cast<int32_t>((uniq[i] >> 21) & 0x1FFFFFu);
      vertices[3 * i + 2] = static_cast<int32_t>(uniq[i] & 0x1FFFFFu);
    }
    for (size_t q = 0; q < n_quads; q++) {
      uint32_t id[4];
      for (int k = 0; k < 4; k++)
        id[k] = static_cast<uint32_t>(std::lower_bound(uniq.begin(), uniq.end(), corner[4 * q + k]) - uniq.begin());
      uint32_t *t = triangles + 6 * q;
      t[0] = id[0]; t[1] = id[1]; t[2] = id[2]; t[3] = id[0]; t[4] = id[2]; t[5] = id[3];
      if (materials) materials[2 * q] = materials[2 * q + 1] = quads[8 * q + 1];
    }
  } catch (const std::bad_alloc &) { return fail("out of memory"); }
  return 0;
}

int tdt_ply_mesh_write(const int32_t *vertices, size_t n_vertices, const uint32_t *triangles, size_t n_triangles, char *buffer,
                       size_t capacity, size_t *bytes) {
  if (!bytes || (n_vertices && !vertices) || (n_triangles && !triangles)) return fail("null argument");
  *bytes = 0;
  for (size_t i = 0; i < 3 * n_vertices; i++)
    if (vertices[i] > static_cast<int32_t>(kCoordMax) || vertices[i] < -static_cast<int32_t>(kCoordMax))
      return fail("vertex " + std::to_string(i / 3) + ": a coordinate beyond +-2^18 units");
  for (size_t i = 0; i < 3 * n_triangles; i++)
    if (triangles[i] >= n_vertices)
      return fail("triangle " + std::to_string(i / 3) + ": vertex index " + std::to_string(triangles[i]) + " >= " + std::to_string(n_vertices) + " vertices");
  try {
    std::string text = "ply\nformat ascii 1.0\nelement vertex " + std::to_string(n_vertices) +
                       "\nproperty float x\nproperty float y\nproperty float z\nelement face " + std::to_string(n_triangles) +
                       "\nproperty list uchar int vertex_indices\nend_header\n";
    char line[96];
    auto coord = [](char *at, int32_t units) {                // units / 64 in decimal, exact: the fraction k / 64 has six digits at most
      const int64_t mag = units < 0 ? -static_cast<int64_t>(units) : units;
      int n = std::sprintf(at, "%s%lld", units < 0 ? "-" : "", static_cast<long long>(mag >> 6));
      const int frac = static_cast<int>(mag & 63) * 15625;   // (k / 64) * 10^6
      if (frac) { n += std::sprintf(at + n, ".%06d", frac); while (at[n - 1] == '0') n--; }
      return n;
    };
    for (size_t i = 0; i < n_vertices; i++) {
      int n = 0;
      for (int d = 0; d < 3; d++) { n += coord(line + n, vertices[3 * i + d]); line[n++] = d < 2 ? ' ' : '\n'; }
      text.append(line, static_cast<size_t>(n));
    }
    for (size_t t = 0; t < n_triangles; t++) {
      const int n = std::sprintf(line, "3 %u %u %u\n", triangles[3 * t], triangles[3 * t + 1], triangles[3 * t + 2]);
      text.append(line, static_cast<size_t>(n));
    }
    *bytes = text.size();
    if (!buffer) return 0;
    if (capacity < text.size()) return fail("capacity " + std::to_string(capacity) + " < " + std::to_string(text.size()) + " bytes");
    std::memcpy(buffer, text.data(), text.size());
  } catch (const std::bad_alloc &) { return fail("out of memory"); }
  return 0;
}

}  // extern "C"
