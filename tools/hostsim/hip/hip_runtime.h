// host stand-in for the HIP constructs the bit-volume units use: one block at a time, 256 real threads, a pthread barrier;
// the block-wide or, the wave shuffle and the wave ballot are called by every thread of the block together
#pragma once
#include <pthread.h>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct int4 { int x, y, z, w; };
struct uint2 { unsigned x, y; };
inline int4 make_int4(int a, int b, int c, int d) { return int4{a, b, c, d}; }
inline thread_local dim3 threadIdx, blockIdx;
typedef int hipError_t; typedef void *hipStream_t; typedef void *hipEvent_t; typedef void *hipDeviceptr_t;
enum { hipSuccess = 0, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
inline hipError_t hipMalloc(void **p, size_t n) { *p = std::malloc(n); return *p ? 0 : 1; }
template <class T> hipError_t hipMalloc(T **p, size_t n) { return hipMalloc((void **)p, n); }
inline hipError_t hipFree(void *p) { std::free(p); return 0; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { std::memcpy(d, s, n); return 0; }
inline hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { std::memset(d, v, n); return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipSetDevice(int) { return 0; }
namespace sim {
inline pthread_barrier_t bar; inline int slot[256]; inline int orv[2]; inline int phase;
inline void sync() { pthread_barrier_wait(&bar); }
}
inline void __syncthreads() { sim::sync(); }
inline int __syncthreads_or(int p) {
  static int acc[2];
  static thread_local int k = 0;
  const int me = k; k ^= 1;
  if (p) __atomic_store_n(&acc[me], 1, __ATOMIC_SEQ_CST);
  sim::sync();
  const int r = __atomic_load_n(&acc[me], __ATOMIC_SEQ_CST);
  sim::sync();
  if (threadIdx.x == 0) acc[me] = 0;
  sim::sync();
  return r;
}
inline int __shfl_xor(int v, int o, int) { sim::slot[threadIdx.x] = v; sim::sync(); const int r = sim::slot[threadIdx.x ^ (unsigned)o]; sim::sync(); return r; }
inline unsigned long long __ballot(int p) {
  sim::slot[threadIdx.x] = p != 0;
  sim::sync();
  unsigned long long r = 0;
  const unsigned w = threadIdx.x & ~63u;
  for (unsigned i = 0; i < 64; i++) r |= (unsigned long long)sim::slot[w + i] << i;
  sim::sync();
  return r;
}
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
inline unsigned atomicOr(unsigned *p, unsigned v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline int atomicMin(int *p, int v) { int o = __atomic_load_n(p, __ATOMIC_SEQ_CST); while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {} return o; }
inline int atomicMax(int *p, int v) { int o = __atomic_load_n(p, __ATOMIC_SEQ_CST); while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {} return o; }
inline unsigned __brev(unsigned x) { unsigned r = 0; for (int i = 0; i < 32; i++) r |= ((x >> i) & 1u) << (31 - i); return r; }
inline int __popc(unsigned x) { return __builtin_popcount(x); }
inline int __ffs(int x) { return __builtin_ffs(x); }
inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
template <class K, class... A> void sim_launch(K k, dim3 g, dim3 b, A... a) {
  pthread_barrier_init(&sim::bar, nullptr, b.x);
  for (unsigned by = 0; by < g.y; by++) for (unsigned bx = 0; bx < g.x; bx++) {
    std::vector<std::thread> t;
    for (unsigned i = 0; i < b.x; i++) t.emplace_back([=]() { threadIdx = dim3(i); blockIdx = dim3(bx, by); k(a...); });
    for (auto &x : t) x.join();
  }
  pthread_barrier_destroy(&sim::bar);
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) sim_launch(k, g, b, __VA_ARGS__)
