// A host stand-in for <hip/hip_runtime.h>, for tests/cxx/points_gradient_host_test.cpp only: the kernels of
// csrc/deform_points_grad.hip compiled as plain C++ and run as workgroups of ONE emulated thread (blockDim.x = 1,
// warpSize = 1, one after the other), so that AddressSanitizer / UndefinedBehaviorSanitizer see every
// index the device code forms.  Dynamic LDS is two fixed arrays whose tail beyond the launch's size is poisoned.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define HOST_HIP_POISON(p, n) __asan_poison_memory_region((p), (n))
#define HOST_HIP_UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef HOST_HIP_POISON
#define HOST_HIP_POISON(p, n) ((void)0)
#define HOST_HIP_UNPOISON(p, n) ((void)0)
#endif

#define __device__
#define __host__
#define __global__
#define __shared__
#define __forceinline__ inline
#define __launch_bounds__(...)

typedef int hipError_t;
typedef void* hipStream_t;
constexpr hipError_t hipSuccess = 0, hipErrorNotSupported = 801, hipErrorOutOfMemory = 2;

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
inline dim3 threadIdx(0, 0, 0), blockIdx(0, 0, 0), blockDim(1, 1, 1), gridDim(1, 1, 1);
constexpr int warpSize = 1;

constexpr size_t kHostLdsBytes = 64 * 1024;
inline size_t host_lds_bytes = 0;               // the running launch's dynamic LDS
void host_lds_begin();                          // (the program's: poisons the LDS arrays beyond host_lds_bytes)

inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
inline void __syncthreads() {}
template <typename T> inline T __shfl_xor(T v, int) { return v; }
inline int __any(int p) { return p; }
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
template <typename T> inline T atomicAdd(T* p, T v) { const T old = *p; *p = old + v; return old; }
template <typename T> inline T atomicMax(T* p, T v) { const T old = *p; *p = old < v ? v : old; return old; }
using std::isfinite;

// The launch as workgroups of ONE thread, one after the other: grid.x * block.x of them, so that a kernel without a
// grid-stride loop still covers its range, and a workgroup's barrier has nobody to wait for.
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                                  \
    do {                                                                                            \
        dim3 host_grid = (grid);                                                                    \
        host_grid.x *= dim3(block).x;                                                               \
        host_lds_bytes = (lds);                                                                     \
        gridDim = host_grid;                                                                        \
        for (unsigned host_y = 0; host_y < host_grid.y; ++host_y)                                   \
            for (unsigned host_x = 0; host_x < host_grid.x; ++host_x) {                             \
                blockIdx = dim3(host_x, host_y, 0);                                                 \
                host_lds_begin();                                                                   \
                kernel(__VA_ARGS__);                                                                \
            }                                                                                       \
    } while (0)
