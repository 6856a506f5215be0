// sam_emu_extra.hpp -- what sam_capi.cpp, sam_subsample_capi.cpp and their kernels use of HIP beyond tests/cxx/hip_emu
// (which stays as it is): the device count, __shfl / __shfl_up, the find-first-set builtins, and launches whose grid has
// a third dimension.  tests/sam_emu.py puts it in front of every translation unit with -include.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return 0; }
inline int __ffs(int v) { return __builtin_ffs(v); }
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
template <typename T> inline T __shfl(T v, int src) {
    const unsigned w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_blk->xch[w][l] = (long long)v; pthread_barrier_wait(&g_blk->wave_bar[w]);
    T r = (T)g_blk->xch[w][src & 63];
    pthread_barrier_wait(&g_blk->wave_bar[w]); return r;
}
template <typename T> inline T __shfl_up(T v, int d) {
    const unsigned w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_blk->xch[w][l] = (long long)v; pthread_barrier_wait(&g_blk->wave_bar[w]);
    T r = (int)l >= d ? (T)g_blk->xch[w][l - d] : v;
    pthread_barrier_wait(&g_blk->wave_bar[w]); return r;
}
// emu_launch of hip_runtime.h with the grid's z: the workgroups one after the other, z outermost
template <typename K, typename... A>
void emu_launch3(K kernel, dim3 grid, dim3 block, A... args) {
    gridDim = grid; blockDim = block;
    EmuBlock blk; g_blk = &blk;
    pthread_barrier_t next_block;
    pthread_barrier_init(&next_block, nullptr, block.x);
    pthread_barrier_init(&blk.block_bar, nullptr, block.x);
    for (unsigned w = 0; w < (block.x + 63) / 64; w++) pthread_barrier_init(&blk.wave_bar[w], nullptr, std::min(64u, block.x - w * 64));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++)
        th.emplace_back([=, &next_block]() {
            for (unsigned bz = 0; bz < grid.z; bz++)
                for (unsigned by = 0; by < grid.y; by++)
                    for (unsigned bx = 0; bx < grid.x; bx++) {
                        threadIdx = dim3(t, 0, 0); blockIdx = dim3(bx, by, bz);
                        kernel(args...);
                        pthread_barrier_wait(&next_block);
                    }
        });
    for (auto& x : th) x.join();
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, lds, s, ...) emu_launch3(k, g, b, __VA_ARGS__)
