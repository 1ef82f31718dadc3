// A stand-in for <hip/hip_runtime.h> that lets a simple translation unit (csrc/gsa_boundary.hip) compile and run on the HOST: a
// workgroup is blockDim.x std::threads that share the function's static "__shared__" arrays and meet at a std::barrier, the
// workgroups of a launch run one after the other.  Only what such a kernel uses: threadIdx / blockIdx (.x), __syncthreads, uint2,
// __umul24, min, hipLaunchKernelGGL on a 1-D grid.  For bounds and logic checks under the host sanitizers (tools/host_emu/
// boundary_asan.cpp); it says nothing about speed, and a kernel that relies on wave-level behaviour cannot use it.
#pragma once
#include <algorithm>
#include <barrier>
#include <cstddef>
#include <cstdint>
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
struct uint2 {
    unsigned x, y;
};
inline uint2 make_uint2(unsigned x, unsigned y) { return uint2{x, y}; }
inline unsigned __umul24(unsigned a, unsigned b) { return (a & 0xffffffu) * (b & 0xffffffu); }
using std::min;
typedef void* hipStream_t;
enum hipError_t { hipSuccess = 0 };
inline hipError_t hipGetLastError() { return hipSuccess; }
template <class K, class... A>
void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, int, hipStream_t, A... args) {
    for (unsigned b = 0; b < grid.x; ++b) {
        emu_barrier.reset(new std::barrier<>(block.x));
        std::vector<std::thread> threads;
        for (unsigned t = 0; t < block.x; ++t)
            threads.emplace_back([=] {
                threadIdx = dim3(t);
                blockIdx = dim3(b);
                kernel(args...);
            });
        for (auto& t : threads) t.join();
    }
}
