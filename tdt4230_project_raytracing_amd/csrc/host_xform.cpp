// Builders of tdt_xform (include/tdt_host.h "affine transforms"): the destination -> source matrix and offset of
// tdt_octree_transform / tdt_octree_extract_transform (include/tdt_rt.h) from the forward transform a caller thinks in.  The
// integer builders are exact; tdt_xform_from_affine and tdt_xform_rotate go through doubles and round.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "tdt_host.h"
#include "tdt_rt.h"

extern "C" void tdt_host_set_error(const char *msg);   // host_scene.cpp

namespace {

constexpr int kInvalidValue = 0x0501;
constexpr long long kOne = TDT_XFORM_ONE, kMaxA = 1ll << 20, kMaxT = 1ll << 40;

int fail(const std::string &m) { tdt_host_set_error(m.c_str()); return kInvalidValue; }

void identity(tdt_xform *x) {
  std::memset(x, 0, sizeof *x);
  x->a[0] = x->a[4] = x->a[8] = (int32_t)kOne;
  x->material = -1;
  for (int i = 0; i < 3; i++) { x->dst_lo[i] = 0; x->dst_hi[i] = INT32_MAX; }
}

// out = the transform with the Q16 inverse matrix a and t = 65536 P - a P, which keeps the doubled point P fixed
int about_pivot(const long long a[9], const int32_t pivot2[3], tdt_xform *out) {
  tdt_xform x;
  identity(&x);
  for (int i = 0; i < 3; i++) {
    __int128 t = (__int128)kOne * pivot2[i];
    for (int j = 0; j < 3; j++) {
      if (a[3 * i + j] > kMaxA || a[3 * i + j] < -kMaxA) return fail("a matrix entry exceeds 2^20 (16.0 in Q16)");
      x.a[3 * i + j] = (int32_t)a[3 * i + j];
      t -= (__int128)a[3 * i + j] * pivot2[j];
    }
    if (t > kMaxT || t < -kMaxT) return fail("the offset exceeds 2^40: the pivot is too far away");
    x.t[i] = (int64_t)t;
  }
  *out = x;
  return 0;
}

}  // namespace

extern "C" {

int tdt_xform_identity(tdt_xform *out) {
  if (!out) return fail("null tdt_xform pointer");
  identity(out);
  return 0;
}

int tdt_xform_translate(const int32_t d[3], tdt_xform *out) {
  if (!d || !out) return fail("null pointer");
  for (int i = 0; i < 3; i++)
    if (d[i] > (1 << 23) || d[i] < -(1 << 23)) return fail("a translation component exceeds 2^23 voxels");
  identity(out);
  for (int i = 0; i < 3; i++) out->t[i] = -(int64_t)d[i] * 131072;
  return 0;
}

int tdt_xform_quarter_turns(int axis, int k, const int32_t pivot2[3], tdt_xform *out) {
  if (!pivot2 || !out) return fail("null pointer");
  if (axis < 0 || axis > 2) return fail("axis must be 0, 1 or 2");
  static const int kCos[4] = {1, 0, -1, 0}, kSin[4] = {0, 1, 0, -1};
  const int turns = ((k % 4) + 4) % 4, c = kCos[turns], s = kSin[turns], u = (axis + 1) % 3, v = (axis + 2) % 3;
  long long a[9] = {};
  a[3 * axis + axis] = kOne;                               // the inverse of the forward turn: its transpose
  a[3 * u + u] = c * kOne; a[3 * u + v] = s * kOne;
  a[3 * v + u] = -s * kOne; a[3 * v + v] = c * kOne;
  return about_pivot(a, pivot2, out);
}

int tdt_xform_mirror(int axis, const int32_t pivot2[3], tdt_xform *out) {
  if (!pivot2 || !out) return fail("null pointer");
  if (axis < 0 || axis > 2) return fail("axis must be 0, 1 or 2");
  long long a[9] = {kOne, 0, 0, 0, kOne, 0, 0, 0, kOne};
  a[3 * axis + axis] = -kOne;
  return about_pivot(a, pivot2, out);
}

int tdt_xform_scale(const int32_t num[3], const int32_t den[3], const int32_t pivot2[3], tdt_xform *out) {
  if (!num || !den || !pivot2 || !out) return fail("null pointer");
  long long a[9] = {};
  for (int i = 0; i < 3; i++) {
    if (num[i] < 1 || den[i] < 1) return fail("num and den must be >= 1");
    a[3 * i + i] = (2 * kOne * den[i] + num[i]) / (2 * (long long)num[i]);   // 65536 den / num, to nearest, halves up
    if (a[3 * i + i] == 0) return fail("the scale exceeds 65536: the matrix would be singular");
  }
  return about_pivot(a, pivot2, out);
}

int tdt_xform_from_affine(const double fwd[12], tdt_xform *out) {
  if (!fwd || !out) return fail("null pointer");
  for (int i = 0; i < 12; i++) if (!std::isfinite(fwd[i])) return fail("the forward transform is not finite");
  const double *F = fwd;                                   // F[4 i + j], j < 3: the matrix; F[4 i + 3]: the offset
  double inv[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {                          // the adjugate
      const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
      inv[3 * r + c] = F[4 * r1 + c1] * F[4 * r2 + c2] - F[4 * r1 + c2] * F[4 * r2 + c1];
    }
  const double det = F[0] * inv[0] + F[1] * inv[3] + F[2] * inv[6];
  if (det == 0.0 || !std::isfinite(det)) return fail("the forward matrix is singular");
  tdt_xform x;
  identity(&x);
  for (int i = 0; i < 3; i++) {
    double t = 0;
    for (int j = 0; j < 3; j++) {
      const double w = inv[3 * i + j] / det;
      const double a = std::rint(65536.0 * w);
      if (!(std::fabs(a) <= (double)kMaxA)) return fail("an entry of the inverse matrix exceeds 16.0");
      x.a[3 * i + j] = (int32_t)a;
      t += w * F[4 * j + 3];
    }
    t = std::rint(-131072.0 * t);
    if (!(std::fabs(t) <= (double)kMaxT)) return fail("the offset exceeds 2^40");
    x.t[i] = (int64_t)t;
  }
  const __int128 d = (__int128)x.a[0] * ((__int128)x.a[4] * x.a[8] - (__int128)x.a[5] * x.a[7]) -
                     (__int128)x.a[1] * ((__int128)x.a[3] * x.a[8] - (__int128)x.a[5] * x.a[6]) +
                     (__int128)x.a[2] * ((__int128)x.a[3] * x.a[7] - (__int128)x.a[4] * x.a[6]);
  if (d == 0) return fail("the inverse matrix is singular once rounded to Q16");
  *out = x;
  return 0;
}

int tdt_xform_rotate(const double axis[3], double degrees, const double pivot[3], tdt_xform *out) {
  if (!axis || !pivot || !out) return fail("null pointer");
  const double len = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
  if (!(len > 0.0) || !std::isfinite(len) || !std::isfinite(degrees)) return fail("the axis must be finite and non-zero");
  const double n[3] = {axis[0] / len, axis[1] / len, axis[2] / len};
  const double rad = degrees * 3.14159265358979323846 / 180.0, c = std::cos(rad), s = std::sin(rad);
  double fwd[12];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {                          // Rodrigues: c I + s [n]x + (1 - c) n n^T
      const int k = 3 - i - j;
      double cross = 0;
      if (i != j) cross = ((j - i + 3) % 3 == 1 ? -1.0 : 1.0) * n[k];
      fwd[4 * i + j] = (i == j ? c : 0.0) + s * cross + (1.0 - c) * n[i] * n[j];
    }
  for (int i = 0; i < 3; i++)
    fwd[4 * i + 3] = pivot[i] - (fwd[4 * i] * pivot[0] + fwd[4 * i + 1] * pivot[1] + fwd[4 * i + 2] * pivot[2]);
  return tdt_xform_from_affine(fwd, out);
}

}  // extern "C"
