#pragma once
// A CPU stand-in for the pieces of HIP that the WEPP entry points use (tests/epp_emu.py, tests/test_sorted_pass_emulation.py).
// Kernels are compiled as plain C++ and run with ONE HOST THREAD PER LANE, in lock step at every cross-lane operation
// (__ballot, __shfl_xor: a barrier per wave; __syncthreads: a barrier per workgroup), one workgroup after the other;
// atomics are the host's.  The runtime is the host's too: device memory is malloc'ed memory, a copy is a memcpy done at
// once, streams and events are tokens that do nothing.  So the host sides of the entry points compile unchanged against it.  It checks
// logic, indexing, buffer sizes and launch order without a GPU; it says nothing about speed, occupancy, the memory
// model of the device or asynchrony between streams.
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
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
struct int4 { int x, y, z, w; };
inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{a, b}; }
typedef int hipError_t; typedef void* hipStream_t; typedef void* hipEvent_t;
constexpr int hipSuccess = 0, hipErrorOutOfMemory = 2;
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
constexpr unsigned hipHostMallocDefault = 0, hipHostMallocPortable = 1, hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000;
constexpr unsigned hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1;
// what is alive: device blocks, host blocks, streams, events (tests/cxx/handle_lifetime_main.cpp: all zero once a
// handle is gone).  emu_malloc_budget: the device allocations that still succeed (negative: all of them).
struct EmuLive { long dev = 0, host = 0, streams = 0, events = 0; };
inline EmuLive g_emu_live;
inline long g_emu_malloc_budget = -1;
inline hipError_t hipGetLastError() { return 0; }
inline const char* hipGetErrorString(hipError_t e) { return e ? "emulated HIP error" : "no error"; }
inline hipError_t hipSetDevice(int) { return 0; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
inline hipError_t hipDeviceSynchronize() { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
// a block is filled with EMU_FILL and followed by a guard of the same: a value read before it was written is
// conspicuous, and a store outside what was asked for can be found afterwards (emu_guard_check, epp_emu.cpp)
constexpr uint32_t EMU_FILL = 0xDEADBEEFu;
constexpr size_t EMU_GUARD_BYTES = 64;
inline hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_emu_malloc_budget == 0) return hipErrorOutOfMemory;
    const size_t words = (bytes + EMU_GUARD_BYTES + 3) / 4;
    uint32_t* w = (uint32_t*)malloc(words * 4);
    if (!w) return hipErrorOutOfMemory;
    if (g_emu_malloc_budget > 0) g_emu_malloc_budget--;
    g_emu_live.dev++;
    std::fill(w, w + words, EMU_FILL);
    *p = w;
    return 0;
}
template <typename T> inline hipError_t hipMalloc(T** p, size_t bytes) { return hipMalloc((void**)p, bytes); }
inline hipError_t hipFree(void* p) { if (p) g_emu_live.dev--; free(p); return 0; }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned = 0) {
    if (!(*p = malloc(bytes))) return hipErrorOutOfMemory;
    g_emu_live.host++;
    return 0;
}
inline hipError_t hipHostFree(void* p) { if (p) g_emu_live.host--; free(p); return 0; }
inline hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) { *dev = host; return 0; }
inline hipError_t hipMemset(void* dst, int v, size_t bytes) { if (bytes) memset(dst, v, bytes); return 0; }
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) { if (bytes) memcpy(dst, src, bytes); return 0; }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind k, hipStream_t) { return hipMemcpy(dst, src, bytes, k); }
inline hipError_t hipMemsetAsync(void* dst, int v, size_t bytes, hipStream_t) { if (bytes) memset(dst, v, bytes); return 0; }
// streams and events are small heap tokens, so that a leak or a second destroy shows under AddressSanitizer; nothing
// looks into them (the null stream is a stream too)
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = malloc(1); g_emu_live.streams++; return 0; }
inline hipError_t hipStreamDestroy(hipStream_t s) { g_emu_live.streams--; free(s); return 0; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = malloc(1); g_emu_live.events++; return 0; }
inline hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDefault); }
inline hipError_t hipEventDestroy(hipEvent_t e) { g_emu_live.events--; free(e); return 0; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return 0; }
inline hipError_t hipEventSynchronize(hipEvent_t) { return 0; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0; return 0; }
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
