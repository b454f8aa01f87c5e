// Host stand-ins for the HIP names that csrc/tg_common.h, csrc/tg_postproc.hip, csrc/tg_coef.hip and csrc/tg_material.hip use, so
// that their kernel source compiles as plain C++ for tools/coef_host_sweep.cpp and tools/material_host_sweep.cpp (address /
// undefined-behaviour sanitizer sweeps on the CPU).
// A launch runs the blocks one after the other with ONE thread each: every loop of these kernels strides by blockDim.x, so
// one thread does the work of the block and the barriers are no-ops.  The dynamic LDS area is a global array of which
// everything beyond the size the launch asked for is poisoned for the address sanitizer.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define TG_HOST_POISON(p, n) __asan_poison_memory_region((p), (n))
#define TG_HOST_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef TG_HOST_POISON
#define TG_HOST_POISON(p, n) ((void)0)
#define TG_HOST_UNPOISON(p, n) ((void)0)
#endif

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__
using std::max;
using std::min;
using std::isfinite;

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
extern dim3 threadIdx, blockIdx, blockDim, gridDim;
#define TG_HOST_LDS_BYTES (160 * 1024)
extern __attribute__((aligned(16))) char smem[];   // what `extern __shared__ char smem[]` of a kernel refers to
extern size_t g_host_lds_max;
static inline void __syncthreads() {}
template <typename T> static inline T __shfl_down(T v, int, int) { return v; }
template <typename T> static inline T __shfl_up(T v, int, int) { return v; }
static inline long long __double_as_longlong(double v) { long long r; memcpy(&r, &v, 8); return r; }
static inline double __longlong_as_double(long long v) { double r; memcpy(&r, &v, 8); return r; }
static inline long long __double2ll_rn(double v) { return llrint(v); }
static inline double __ll2double_rn(long long v) { return (double)v; }
template <typename T> static inline T atomicAdd(T *p, T v) { T o = *p; *p += v; return o; }
template <typename T> static inline T atomicMin(T *p, T v) { T o = *p; if (v < o) *p = v; return o; }
static inline double unsafeAtomicAdd(double *p, double v) { double o = *p; *p += v; return o; }

typedef int hipError_t;
enum { hipSuccess = 0 };
typedef void *hipStream_t;
typedef void *hipEvent_t;
enum { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
enum { hipFuncAttributeMaxDynamicSharedMemorySize };
static inline const char *hipGetErrorString(hipError_t) { return "host build"; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static inline hipError_t hipFuncSetAttribute(const void *, int, int) { return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }

template <typename F>
static inline void tg_host_launch(F &&body, dim3 grid, size_t lds) {
  if (lds > TG_HOST_LDS_BYTES) abort();
  g_host_lds_max = std::max(g_host_lds_max, lds);
  TG_HOST_POISON(smem + lds, TG_HOST_LDS_BYTES - lds);
  blockDim = dim3(1);
  gridDim = grid;                 // (kernels that stride over a capped grid: csrc/tg_sample.hip)
  threadIdx = dim3(0, 0, 0);
  for (unsigned b = 0; b < grid.x; b++) {
    blockIdx = dim3(b, 0, 0);
    body();
  }
  TG_HOST_UNPOISON(smem, TG_HOST_LDS_BYTES);
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) tg_host_launch([&] { kernel(__VA_ARGS__); }, grid, lds)
