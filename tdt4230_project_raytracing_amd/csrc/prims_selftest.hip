// Test-only harness over the two device primitives every octree operation is built on: exclusive_scan_u32
// (device_scan.hpp, compiled here from the same header the product includes) and tdt::sort_pairs_u32 (tdt_build.hip,
// resolved from libtdtrt.so at load time, so the sort under test is the product's own).  Built as
// libtdtprims_selftest.so next to libtdtrt.so; it is not part of the C ABI and nothing in the product calls it.
//
// Every device array is one allocation of [front words][payload][kGuardWords guard words].  The payload starts 4 + skew
// words into the allocation (skew 0: 16-byte aligned, as a hipMalloc pointer is); the front and guard words hold
// canary(j), j counted from the payload's end for the guards and backwards from its start for the front.  Scratch arrays
// are exactly as long as the product's own sizing functions say, so a primitive that writes past what its caller was
// told to allocate changes a canary instead of faulting.  The canaries go back to the caller, which asserts them.
#include <cstdint>
#include <cstring>

#include "device_scan.hpp"
#include "tdt_internal.hpp"

namespace {

// 512 guard words: a histogram sized for one sort tile too few overruns by 256 words, and that must stay inside the allocation
constexpr uint32_t kGuardWords = 512, kFrontWords = 4, kMaxSkew = 3;
constexpr uint32_t kReport = kFrontWords + kGuardWords;       // canary words reported per array: front, then guards
inline uint32_t canary(uint32_t j) { return 0xC5A70000u + j; }

struct Guarded {               // one device array and its host image
  uint32_t *base = nullptr, *host = nullptr;
  size_t words = 0, total = 0;
  uint32_t skew = 0;
  ~Guarded() { if (base) (void)hipFree(base); delete[] host; }
  uint32_t *dev() const { return base + kFrontWords + skew; }
  // allocate, fill front / guards with canaries and the payload with `data` (null: a junk pattern), upload
  hipError_t create(size_t n, uint32_t skew_words, const uint32_t *data) {
    words = n; skew = skew_words; total = kFrontWords + skew + n + kGuardWords;
    host = new uint32_t[total];
    const size_t front = kFrontWords + skew;
    for (size_t j = 0; j < front; j++) host[front - 1 - j] = canary((uint32_t)j);
    if (data) { if (n) memcpy(host + front, data, n * sizeof(uint32_t)); }
    else for (size_t j = 0; j < n; j++) host[front + j] = 0xDEAD0000u ^ (uint32_t)j;
    for (size_t j = 0; j < kGuardWords; j++) host[front + n + j] = canary((uint32_t)j);
    hipError_t e = hipMalloc((void **)&base, total * sizeof(uint32_t));
    if (e != hipSuccess) { base = nullptr; return e; }
    return hipMemcpy(base, host, total * sizeof(uint32_t), hipMemcpyHostToDevice);
  }
  // download; payload into `payload` (may be null), the kFrontWords words before it and the guards after it into `report`
  hipError_t fetch(uint32_t *payload, uint32_t *report) {
    const hipError_t e = hipMemcpy(host, base, total * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    const size_t front = kFrontWords + skew;
    if (payload && words) memcpy(payload, host + front, words * sizeof(uint32_t));
    for (size_t j = 0; j < kFrontWords; j++) report[j] = host[front - 1 - j];
    memcpy(report + kFrontWords, host + front + words, kGuardWords * sizeof(uint32_t));
    return hipSuccess;
  }
};

void untouched(uint32_t *report) {   // what an array that was never allocated reports
  for (uint32_t j = 0; j < kFrontWords; j++) report[j] = canary(j);
  for (uint32_t j = 0; j < kGuardWords; j++) report[kFrontWords + j] = canary(j);
}

#define ST_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return (int)e_; } while (0)

}  // namespace

extern "C" {

// canary words reported per array (front words first, then the guard words) and the value of word j, for the caller's assertions
uint32_t selftest_guard_report_words(void) { return kReport; }
uint32_t selftest_front_words(void) { return kFrontWords; }
uint32_t selftest_canary(uint32_t j) { return canary(j); }

// out[0..n) = exclusive_scan_u32 of in[0..n) on the device.  in_place != 0: one array serves as both (skew_out applies).
// in_after[0..n): the input array as it is after the scan (in_place: the same as out).  guards: 3 reports of
// selftest_guard_report_words() words — in, out, scratch.  Returns the hipError_t, 0 on success.
int selftest_scan_u32(const uint32_t *in, uint32_t *out, uint32_t n, int in_place, uint32_t skew_in, uint32_t skew_out,
                      uint32_t skew_scratch, uint32_t *in_after, uint32_t *guards) {
  if (skew_in > kMaxSkew || skew_out > kMaxSkew || skew_scratch > kMaxSkew) return (int)hipErrorInvalidValue;
  Guarded d_in, d_out, d_scr;
  if (!in_place) ST_HIP(d_in.create(n, skew_in, in));
  ST_HIP(d_out.create(n, skew_out, in_place ? in : nullptr));
  ST_HIP(d_scr.create(tdt::scan_scratch_words(n), skew_scratch, nullptr));
  ST_HIP(tdt::exclusive_scan_u32(nullptr, in_place ? d_out.dev() : d_in.dev(), d_out.dev(), n, d_scr.dev()));
  ST_HIP(hipStreamSynchronize(nullptr));
  ST_HIP(d_out.fetch(out, guards + kReport));
  if (in_place) { untouched(guards); if (n) memcpy(in_after, out, (size_t)n * sizeof(uint32_t)); }
  else ST_HIP(d_in.fetch(in_after, guards));
  ST_HIP(d_scr.fetch(nullptr, guards + 2 * kReport));
  return 0;
}

// (keys_out, vals_out)[0..n) = tdt::sort_pairs_u32 of (keys, vals)[0..n).  guards: 6 reports — the two key arrays, the two
// value arrays, hist (sort_hist_words(n) words), scratch (sort_scratch_words(n) words).
int selftest_sort_pairs_u32(const uint32_t *keys, const uint32_t *vals, uint32_t n, uint32_t *keys_out, uint32_t *vals_out,
                            uint32_t *guards) {
  Guarded k0, k1, v0, v1, hist, scr;
  ST_HIP(k0.create(n, 0, keys));
  ST_HIP(k1.create(n, 0, nullptr));
  ST_HIP(v0.create(n, 0, vals));
  ST_HIP(v1.create(n, 0, nullptr));
  ST_HIP(hist.create(tdt::sort_hist_words(n), 0, nullptr));
  ST_HIP(scr.create(tdt::sort_scratch_words(n), 0, nullptr));
  uint32_t *k = k0.dev(), *v = v0.dev();
  ST_HIP(tdt::sort_pairs_u32(nullptr, k, v, k1.dev(), v1.dev(), n, hist.dev(), scr.dev()));
  ST_HIP(hipStreamSynchronize(nullptr));
  if ((k != k0.dev() && k != k1.dev()) || (v != v0.dev() && v != v1.dev())) return (int)hipErrorUnknown;
  ST_HIP(k0.fetch(k == k0.dev() ? keys_out : nullptr, guards));
  ST_HIP(k1.fetch(k == k1.dev() ? keys_out : nullptr, guards + kReport));
  ST_HIP(v0.fetch(v == v0.dev() ? vals_out : nullptr, guards + 2 * kReport));
  ST_HIP(v1.fetch(v == v1.dev() ? vals_out : nullptr, guards + 3 * kReport));
  ST_HIP(hist.fetch(nullptr, guards + 4 * kReport));
  ST_HIP(scr.fetch(nullptr, guards + 5 * kReport));
  return 0;
}

}  // extern "C"
