#pragma once
// A CPU stand-in for the few pieces of the HIP runtime that assign_kernels.hip uses, for tests/test_assign_emulation.py:
// the kernels are compiled as plain C++ and run with ONE HOST THREAD PER LANE, in lock step at every cross-lane
// operation (__ballot, __shfl_xor: a barrier per wave; __syncthreads: a barrier per workgroup), one workgroup after the
// other.  Atomics are the host's.  It checks the kernels' logic and indexing without a GPU; it says nothing about
// speed, occupancy or the memory model of the device.
#include <pthread.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __shared__ static
// dynamic LDS: one workgroup runs at a time, so one host buffer serves
extern unsigned char g_emu_lds[];
#define HIP_DYNAMIC_SHARED(type, var) type* var = (type*)g_emu_lds;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint2 { uint32_t x, y; };
inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{a, b}; }
typedef int hipError_t; typedef void* hipStream_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
extern thread_local dim3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;
using std::min; using std::max;
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
template <typename T> inline T __builtin_amdgcn_readfirstlane(T v) { return v; }
template <typename T> inline T __hip_atomic_load(T* p, int, int) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
template <typename T, typename U> inline T atomicAdd(T* p, U v) { return __atomic_fetch_add(p, (T)v, __ATOMIC_RELAXED); }
template <typename T> inline T atomicOr(T* p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
template <typename T> inline T atomicMax(T* p, T v) { T o = __atomic_load_n(p, __ATOMIC_RELAXED); while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} return o; }
// wave / block emulation: one std::thread per lane, lock-step at every cross-lane operation
struct EmuBlock { pthread_barrier_t block_bar; pthread_barrier_t wave_bar[16]; long long xch[16][64]; };
extern EmuBlock* g_blk;
inline void __syncthreads() { pthread_barrier_wait(&g_blk->block_bar); }
inline unsigned long long __ballot(bool p) {
    const unsigned w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_blk->xch[w][l] = p; pthread_barrier_wait(&g_blk->wave_bar[w]);
    unsigned long long r = 0; for (int i = 0; i < 64; i++) r |= (unsigned long long)(g_blk->xch[w][i] & 1) << i;
    pthread_barrier_wait(&g_blk->wave_bar[w]); return r;
}
template <typename T> inline T __shfl_xor(T v, int o) {
    const unsigned w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_blk->xch[w][l] = (long long)v; pthread_barrier_wait(&g_blk->wave_bar[w]);
    T r = (T)g_blk->xch[w][l ^ o];
    pthread_barrier_wait(&g_blk->wave_bar[w]); return r;
}
// the lanes of a workgroup are host threads that live for the whole launch and take its workgroups one after the other
template <typename K, typename... A>
void emu_launch(K kernel, dim3 grid, dim3 block, A... args) {
    gridDim = grid; blockDim = block;
    EmuBlock blk; g_blk = &blk;
    pthread_barrier_t next_block;
    pthread_barrier_init(&next_block, nullptr, block.x);
    pthread_barrier_init(&blk.block_bar, nullptr, block.x);
    for (unsigned w = 0; w < (block.x + 63) / 64; w++) pthread_barrier_init(&blk.wave_bar[w], nullptr, std::min(64u, block.x - w * 64));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++)
        th.emplace_back([=, &next_block]() {
            for (unsigned by = 0; by < grid.y; by++)
                for (unsigned bx = 0; bx < grid.x; bx++) {
                    threadIdx = dim3(t); blockIdx = dim3(bx, by);
                    kernel(args...);
                    pthread_barrier_wait(&next_block);
                }
        });
    for (auto& x : th) x.join();
}
#define hipLaunchKernelGGL(k, g, b, lds, s, ...) emu_launch(k, g, b, __VA_ARGS__)
