// geno_kernels.hip -- the device side of wepp_geno_diameters and wepp_geno_nearest (geno.hpp): columns, bit-planes
// and the two pair forms.  Everything is exact integer work; the reductions are atomicMax / atomicMin / atomicOr on
// integers, so a result does not depend on the order the workgroups run in.  rocPRIM is used for one stable radix
// sort of pairs and exclusive scans only (what tests/cxx/hip_emu stands in for).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "geno.hpp"

namespace wepp {
namespace {

typedef unsigned long long u64;

inline uint32_t blocks_for(u64 n) { return (uint32_t)std::min<u64>(std::max<u64>((n + GENO_BLOCK - 1) / GENO_BLOCK, 1), 1u << 16); }

// the number of a[0 .. n) that are <= v (a ascends)
template <typename T>
__device__ __forceinline__ uint32_t count_le(const T* a, uint32_t n, T v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_geno_keys(GenoWords w, u64* key, uint32_t* val) {
    for (u64 i = (u64)blockIdx.x * GENO_BLOCK + threadIdx.x; i < w.n_words; i += (u64)gridDim.x * GENO_BLOCK) {
        const uint32_t word = w.item_word[i], pos = word & ((1u << GENO_POS_BITS) - 1);
        const uint32_t item = count_le<u64>(w.item_off, w.n_items + 1, i) - 1;
        const uint32_t set = w.set_off ? count_le<uint32_t>(w.set_off, w.n_sets + 1, item) - 1 : 0;
        const bool drop = w.keep_bits && (pos >= w.keep_positions || !((w.keep_bits[pos >> 5] >> (pos & 31)) & 1));
        key[i] = drop ? (u64)w.n_sets << GENO_POS_BITS : ((u64)set << GENO_POS_BITS) | pos;
        val[i] = (uint32_t)i;
    }
}

__global__ void k_geno_heads(const u64* key, u64 n, uint32_t n_sets, uint32_t* head) {
    for (u64 j = (u64)blockIdx.x * GENO_BLOCK + threadIdx.x; j <= n; j += (u64)gridDim.x * GENO_BLOCK) {
        uint32_t h = 0;
        if (j < n) {
            const u64 k = key[j];
            h = (k >> GENO_POS_BITS) < n_sets && (j == 0 || key[j - 1] != k);
        }
        head[j] = h;
    }
}

__global__ void k_geno_sets(const u64* key, const uint32_t* head, const uint32_t* rank, u64 n, uint32_t n_sets, uint32_t* set_first,
                            uint32_t* set_cols) {
    for (u64 j = (u64)blockIdx.x * GENO_BLOCK + threadIdx.x; j < n; j += (u64)gridDim.x * GENO_BLOCK) {
        if (!head[j]) continue;
        const u64 s = key[j] >> GENO_POS_BITS;
        atomicAdd(&set_cols[s], 1u);
        if (j == 0 || (key[j - 1] >> GENO_POS_BITS) != s) set_first[s] = rank[j];   // (heads before j = this column's global index)
    }
}

__global__ void k_geno_word_cols(const u64* key, const uint32_t* val, const uint32_t* head, const uint32_t* rank, u64 n, uint32_t n_sets,
                                 const uint32_t* set_first, uint32_t* word_col) {
    for (u64 j = (u64)blockIdx.x * GENO_BLOCK + threadIdx.x; j < n; j += (u64)gridDim.x * GENO_BLOCK) {
        const u64 s = key[j] >> GENO_POS_BITS;
        word_col[val[j]] = s < n_sets ? rank[j] + head[j] - 1 - set_first[s] : GENO_NO_COLUMN;
    }
}

__global__ void k_geno_planes(GenoWords w, const uint32_t* word_col, GenoPass p, u64 first_word, u64 end_word) {
    for (u64 i = first_word + (u64)blockIdx.x * GENO_BLOCK + threadIdx.x; i < end_word; i += (u64)gridDim.x * GENO_BLOCK) {
        const uint32_t col = word_col[i];
        if (col == GENO_NO_COLUMN) continue;
        const uint32_t item = count_le<u64>(w.item_off, w.n_items + 1, i) - 1;
        const uint32_t s = count_le<uint32_t>(p.set_item0, p.n_sets, item) - 1;   // (empty sets share their first item with the next set: the last one wins)
        const uint32_t W = p.set_words[s];
        if (W == 0) continue;   // (a set the pass keeps no planes of)
        const u64 at = p.set_base[s] + ((u64)(item - p.set_item0[s]) * W + (col >> 6)) * 4;
        const uint32_t mut = (w.item_word[i] >> 24) & 15;
        for (uint32_t b = 0; b < 4; b++)
            if ((mut >> b) & 1) atomicOr(&p.planes[at + b], 1ull << (col & 63));
    }
}

__device__ __forceinline__ int wave_max(int v) {
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// one wave per set of 2 .. GENO_WAVE_ITEMS items, the lanes over its ordered pairs (i, j), i < j; the planes are read
// from global memory (such a set has few columns)
__global__ void __launch_bounds__(GENO_BLOCK) k_geno_wave(GenoPass p, const uint32_t* small, uint32_t n_small, int32_t* diam) {
    const uint32_t k = blockIdx.x * (GENO_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= n_small) return;   // (the whole wave)
    const uint32_t s = small[k], n = p.set_items[s], W = p.set_words[s];
    const u64* pl = p.planes + p.set_base[s];
    int best = 0;
    for (uint32_t idx = lane; idx < n * n; idx += 64) {
        const uint32_t i = idx / n, j = idx % n;
        if (i >= j) continue;
        const u64 *a = pl + (u64)i * W * 4, *b = pl + (u64)j * W * 4;
        int d = 0;
        for (uint32_t w = 0; w < W * 4; w += 4) d += __popcll((a[w] ^ b[w]) | (a[w + 1] ^ b[w + 1]) | (a[w + 2] ^ b[w + 2]) | (a[w + 3] ^ b[w + 3]));
        best = max(best, d);
    }
    best = wave_max(best);
    if (lane == 0) atomicMax(&diam[p.set0 + s], best);
}

// One workgroup per tile of GENO_TILE x GENO_TILE pairs: lane = the row item, each of the four waves takes 16 of the
// column items.  Both tiles' planes are staged in LDS, GENO_CHUNK_WORDS column words at a time: the row tile with the
// item as the fast index (a wave reads consecutive 8-byte words), the column tile item-major (a wave reads one
// address: a broadcast).
template <bool NEAREST>
__global__ void __launch_bounds__(GENO_BLOCK) k_geno_tile(GenoPass p, const GenoTileJob* jobs, uint32_t n_a, int32_t* diam, u64* best, int32_t* matrix) {
    constexpr uint32_t CW4 = GENO_CHUNK_WORDS * 4, PER_WAVE = GENO_TILE / (GENO_BLOCK / 64);
    __shared__ u64 sA[CW4 * GENO_TILE_PAD];
    __shared__ u64 sB[GENO_TILE * CW4];
    const GenoTileJob job = jobs[blockIdx.x];
    const uint32_t s = job.set, W = p.set_words[s], n = p.set_items[s];
    const u64* pl = p.planes + p.set_base[s];
    const uint32_t rows = NEAREST ? n_a : n, row0 = job.ti * GENO_TILE, col_first = NEAREST ? n_a : 0, col0 = job.tj * GENO_TILE;
    const uint32_t na = min(GENO_TILE, rows - row0), nb = min(GENO_TILE, n - col_first - col0);
    const uint32_t t = threadIdx.x, a = t & 63, wv = t >> 6;
    int acc[PER_WAVE];
    for (uint32_t k = 0; k < PER_WAVE; k++) acc[k] = 0;
    for (uint32_t w0 = 0; w0 < W; w0 += GENO_CHUNK_WORDS) {
        __syncthreads();   // (the chunk before this one has been read)
        for (uint32_t e = t; e < GENO_TILE * CW4; e += GENO_BLOCK) {
            const uint32_t item = e / CW4, rem = e % CW4;
            const bool in_w = w0 + rem / 4 < W;
            sA[rem * GENO_TILE_PAD + item] = item < na && in_w ? pl[((u64)(row0 + item) * W + w0) * 4 + rem] : 0;
            sB[item * CW4 + rem] = item < nb && in_w ? pl[((u64)(col_first + col0 + item) * W + w0) * 4 + rem] : 0;
        }
        __syncthreads();
        for (uint32_t w = 0; w < CW4; w += 4) {
            const u64 x0 = sA[w * GENO_TILE_PAD + a], x1 = sA[(w + 1) * GENO_TILE_PAD + a], x2 = sA[(w + 2) * GENO_TILE_PAD + a],
                      x3 = sA[(w + 3) * GENO_TILE_PAD + a];
            for (uint32_t k = 0; k < PER_WAVE; k++) {
                const u64* y = sB + (wv * PER_WAVE + k) * CW4 + w;
                acc[k] += __popcll((x0 ^ y[0]) | (x1 ^ y[1]) | (x2 ^ y[2]) | (x3 ^ y[3]));
            }
        }
    }
    if (NEAREST) {
        u64 m = ~0ull;
        for (uint32_t k = 0; k < PER_WAVE; k++) {
            const uint32_t b = wv * PER_WAVE + k;
            if (a >= na || b >= nb) continue;
            m = min(m, ((u64)(uint32_t)acc[k] << 32) | (col0 + b));
            if (matrix) matrix[(u64)(row0 + a) * (n - n_a) + col0 + b] = acc[k];
        }
        if (m != ~0ull) atomicMin(&best[row0 + a], m);
    } else {
        int m = 0;
        for (uint32_t k = 0; k < PER_WAVE; k++)
            if (a < na && wv * PER_WAVE + k < nb) m = max(m, acc[k]);   // (an item against itself gives 0)
        m = wave_max(m);
        if (a == 0) atomicMax(&diam[p.set0 + s], m);
    }
}

}  // namespace

hipError_t launch_geno_keys(const GenoWords& w, unsigned long long* key, uint32_t* val, hipStream_t stream) {
    if (w.n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_geno_keys, dim3(blocks_for(w.n_words)), dim3(GENO_BLOCK), 0, stream, w, key, val);
    return hipGetLastError();
}

hipError_t geno_sort_temp_bytes(unsigned long long n, uint32_t key_bits, size_t* bytes) {
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, (const u64*)nullptr, (u64*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0,
                                     key_bits, nullptr);
}

hipError_t launch_geno_sort(const unsigned long long* key_in, unsigned long long* key_out, const uint32_t* val_in, uint32_t* val_out,
                            unsigned long long n, uint32_t key_bits, void* temp, size_t temp_bytes, hipStream_t stream) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, key_in, key_out, val_in, val_out, (size_t)n, 0, key_bits, stream);
}

hipError_t launch_geno_heads(const unsigned long long* key, unsigned long long n, uint32_t n_sets, uint32_t* head, hipStream_t stream) {
    hipLaunchKernelGGL(k_geno_heads, dim3(blocks_for(n + 1)), dim3(GENO_BLOCK), 0, stream, key, n, n_sets, head);
    return hipGetLastError();
}

hipError_t geno_scan_temp_bytes(unsigned long long n, size_t* bytes) {
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), nullptr);
}

hipError_t launch_geno_scan(const uint32_t* head, uint32_t* rank, unsigned long long n, void* temp, size_t temp_bytes, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, temp_bytes, head, rank, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), stream);
}

hipError_t launch_geno_sets(const unsigned long long* key, const uint32_t* head, const uint32_t* rank, unsigned long long n, uint32_t n_sets,
                            uint32_t* set_first, uint32_t* set_cols, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_geno_sets, dim3(blocks_for(n)), dim3(GENO_BLOCK), 0, stream, key, head, rank, n, n_sets, set_first, set_cols);
    return hipGetLastError();
}

hipError_t launch_geno_word_cols(const unsigned long long* key, const uint32_t* val, const uint32_t* head, const uint32_t* rank,
                                 unsigned long long n, uint32_t n_sets, const uint32_t* set_first, uint32_t* word_col, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_geno_word_cols, dim3(blocks_for(n)), dim3(GENO_BLOCK), 0, stream, key, val, head, rank, n, n_sets, set_first, word_col);
    return hipGetLastError();
}

hipError_t launch_geno_planes(const GenoWords& w, const uint32_t* word_col, const GenoPass& p, unsigned long long first_word,
                              unsigned long long end_word, hipStream_t stream) {
    if (end_word <= first_word) return hipSuccess;
    hipLaunchKernelGGL(k_geno_planes, dim3(blocks_for(end_word - first_word)), dim3(GENO_BLOCK), 0, stream, w, word_col, p, first_word, end_word);
    return hipGetLastError();
}

hipError_t launch_geno_wave(const GenoPass& p, const uint32_t* small, uint32_t n_small, int32_t* diam, hipStream_t stream) {
    if (n_small == 0) return hipSuccess;
    constexpr uint32_t per_block = GENO_BLOCK / 64;
    hipLaunchKernelGGL(k_geno_wave, dim3((n_small + per_block - 1) / per_block), dim3(GENO_BLOCK), 0, stream, p, small, n_small, diam);
    return hipGetLastError();
}

hipError_t launch_geno_tile_diam(const GenoPass& p, const GenoTileJob* jobs, uint32_t n_jobs, int32_t* diam, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_geno_tile<false>, dim3(n_jobs), dim3(GENO_BLOCK), 0, stream, p, jobs, 0u, diam, (u64*)nullptr, (int32_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_geno_tile_nearest(const GenoPass& p, const GenoTileJob* jobs, uint32_t n_jobs, uint32_t n_a, unsigned long long* best,
                                    int32_t* matrix, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_geno_tile<true>, dim3(n_jobs), dim3(GENO_BLOCK), 0, stream, p, jobs, n_a, (int32_t*)nullptr, best, matrix);
    return hipGetLastError();
}

}  // namespace wepp
