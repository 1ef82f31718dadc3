// A stand-in for <hip/hip_runtime.h> that lets the stateless tile kernels (csrc/gsa_boundary.hip, gsa_mask.hip, gsa_augment.hip,
// gsa_photometric.hip) compile and run on the HOST, unedited: a launch is blockDim.x std::threads, created once, that walk the
// workgroups of the grid in order; inside a workgroup they share the function's static "__shared__" arrays and meet at a
// std::barrier, and they meet at it once more between one workgroup and the next, because those arrays are reused.  Only what such
// a kernel uses: threadIdx / blockIdx (.x), __syncthreads, the vector types with HIP's alignment, __umul24, __umulhi,
// __float_as_uint, v_sad_u8, min, <cmath>, hipLaunchKernelGGL on a 1-D grid.  For bounds, alignment, arithmetic and barrier checks
// under the host sanitizers (tools/host_emu/emu_run.cpp, tests/test_host_emu.py); it says nothing about speed, nothing about what
// happens between workgroups, and a kernel that relies on wave-level behaviour (ballot, shuffle, readlane) cannot use it.  A thread
// that returns from the kernel waits for the next workgroup: a __syncthreads() that not every thread reaches hangs here.
#pragma once
#include <math.h>

#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
inline thread_local dim3 threadIdx, blockIdx;
inline std::unique_ptr<std::barrier<>> emu_barrier;
inline void __syncthreads() { emu_barrier->arrive_and_wait(); }
// the vector types, aligned as HIP aligns them: an access through a reinterpret_cast at a lesser address is UBSan's to report
struct alignas(8) uint2 {
    unsigned x, y;
};
struct alignas(16) uint4 {
    unsigned x, y, z, w;
};
struct alignas(8) ushort4 {
    unsigned short x, y, z, w;
};
struct alignas(16) float4 {
    float x, y, z, w;
};
inline uint2 make_uint2(unsigned x, unsigned y) { return uint2{x, y}; }
inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }
inline ushort4 make_ushort4(unsigned short x, unsigned short y, unsigned short z, unsigned short w) { return ushort4{x, y, z, w}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline unsigned __umul24(unsigned a, unsigned b) { return (a & 0xffffffu) * (b & 0xffffffu); }
inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
inline unsigned __float_as_uint(float v) {
    unsigned u;
    std::memcpy(&u, &v, 4);
    return u;
}
inline float __uint_as_float(unsigned u) {
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}
// v_sad_u8: acc + the sum of the four absolute byte differences
inline unsigned __builtin_amdgcn_sad_u8(unsigned a, unsigned b, unsigned acc) {
    for (int k = 0; k < 4; ++k) {
        const int x = (int)((a >> (8 * k)) & 255u), y = (int)((b >> (8 * k)) & 255u);
        acc += (unsigned)(x > y ? x - y : y - x);
    }
    return acc;
}
using std::min;
typedef void* hipStream_t;
enum hipError_t { hipSuccess = 0 };
inline hipError_t hipGetLastError() { return hipSuccess; }
template <class K, class... A>
void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, int, hipStream_t, A... args) {
    emu_barrier.reset(new std::barrier<>(block.x));
    std::vector<std::thread> threads;
    for (unsigned t = 0; t < block.x; ++t)
        threads.emplace_back([=] {
            threadIdx = dim3(t);
            for (unsigned b = 0; b < grid.x; ++b) {     // workgroups one after the other
                blockIdx = dim3(b);
                kernel(args...);
                emu_barrier->arrive_and_wait();         // the next workgroup reuses the "shared" arrays
            }
        });
    for (auto& t : threads) t.join();
}
