// sam_kernels.hip -- the device side of wepp_sam_build (sam.hpp; host side sam_capi.cpp): the pile-up of every aligned
// column into the per-site table, the keep table of the read correction, the reads' words, the exact sort of the
// corrected reads and their merge.  Integers throughout, except the one fp64 expression of the correction, which is
// evaluated once per table cell exactly as the reference writes it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "sam.hpp"

namespace wepp {
namespace {

using u64 = unsigned long long;

__device__ __forceinline__ u64 shfl64(u64 v, int lane) {
    const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// ---- pile-up ---------------------------------------------------------------------------------------------------------
// Workgroup (t, k) owns tile t of SAM_TILE sites and chunk k of the reads.  A wave looks at 64 read windows at a time,
// keeps those that meet the tile and adds their columns inside it into the tile's counters in LDS, a lane per column
// (the lanes of one instruction hit distinct sites).  Non-zero counters then go to the table with one global atomic
// each: the table sees a few atomics per cell and workgroup, not one per aligned column.
__global__ __launch_bounds__(SAM_BLOCK) void k_sam_pileup(SamReadsDev rd, uint32_t reads_per_chunk, uint32_t* __restrict__ freq,
                                                           uint32_t* __restrict__ bad_base) {
    __shared__ uint32_t cnt[SAM_TILE * 6];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < SAM_TILE * 6; i += SAM_BLOCK) cnt[i] = 0;
    __syncthreads();
    const uint32_t tile_lo = blockIdx.x * SAM_TILE, tile_hi = min(rd.G, tile_lo + SAM_TILE);
    const u64 r0 = (u64)blockIdx.y * reads_per_chunk, r1 = min((u64)rd.R, r0 + reads_per_chunk);
    bool bad = false;
    for (u64 rb = r0 + wave * 64; rb < r1; rb += SAM_BLOCK) {
        const u64 r = rb + lane;
        uint32_t s = 0, len = 0;
        u64 o = 0;
        if (r < r1) { s = rd.start[r]; o = rd.base_off[r]; len = (uint32_t)(rd.base_off[r + 1] - o); }
        u64 meets = __ballot(len != 0 && s < tile_hi && s + len > tile_lo);
        while (meets) {
            const int l = __ffsll((long long)meets) - 1;
            meets &= meets - 1;
            const uint32_t rs = __shfl(s, l), rlen = __shfl(len, l);
            const u64 ro = shfl64(o, l);
            const uint32_t lo = max(rs, tile_lo), hi = min(rs + rlen, tile_hi);
            for (uint32_t p = lo + lane; p < hi; p += 64) {
                const uint32_t c = rd.base[ro + (p - rs)];
                if (c > SAM_CODE_GAP) bad = true;
                else if (c != SAM_CODE_N) atomicAdd(&cnt[(p - tile_lo) * 6 + c], 1u);
            }
        }
    }
    if (bad) *bad_base = 1;
    __syncthreads();
    const uint32_t cells = (tile_hi - tile_lo) * 6;
    for (uint32_t i = tid; i < cells; i += SAM_BLOCK) {
        const uint32_t v = cnt[i];
        if (v) atomicAdd(&freq[(u64)tile_lo * 6 + i], v);
    }
}

// ---- keep table ------------------------------------------------------------------------------------------------------
// sam::read_correction, sam2pb.cpp:297-312, per cell instead of per aligned column
__global__ __launch_bounds__(SAM_BLOCK) void k_sam_keep(const uint32_t* __restrict__ freq, uint32_t G, double min_af, uint32_t min_depth,
                                                         uint8_t* __restrict__ keep) {
    const uint32_t site = blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (site >= G) return;
    uint32_t f[6];
    long long total = 0;
    for (int c = 0; c < 6; c++) { f[c] = freq[(u64)site * 6 + c]; total += f[c]; }
    for (uint32_t c = 0; c < 6; c++) {
        uint32_t k = c;
        if ((long long)min_depth > total) k = SAM_CODE_N;
        else if (min_af - (double)f[c] / (double)total > 1e-9) k = SAM_CODE_N;
        if (k == SAM_CODE_GAP) k = SAM_CODE_N;
        keep[(u64)site * 6 + c] = (uint8_t)k;
    }
}

// ---- the reads' words ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t code_char(uint32_t k) { return k == 0 ? 'A' : k == 1 ? 'C' : k == 2 ? 'G' : k == 3 ? 'T' : 'N'; }
__device__ __forceinline__ uint32_t code_mask(uint32_t k) { return k < 4 ? 1u << k : 15u; }
__device__ __forceinline__ uint32_t char_mask(uint32_t ch) {      // MAT::get_nuc_id
    switch (ch) {
    case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'G': case 'g': return 4; case 'T': case 't': return 8;
    case 'R': return 5; case 'Y': return 10; case 'S': return 6; case 'W': return 9; case 'K': return 12; case 'M': return 3;
    case 'B': return 14; case 'D': return 13; case 'H': return 11;
    default: return 15;
    }
}
__device__ __forceinline__ uint32_t pack_word(uint32_t position, uint32_t ref_nuc, uint32_t mut_nuc, uint32_t is_missing) {   // wepp_pack_read_word
    return (position & 0xFFFFFu) | ((ref_nuc & 15u) << 20) | ((mut_nuc & 15u) << 24) | ((is_missing & 1u) << 28);
}

// one wave per read; with words == nullptr only the count is written
__global__ __launch_bounds__(SAM_BLOCK) void k_sam_words(SamReadsDev rd, const uint8_t* __restrict__ keep, uint32_t* __restrict__ n_words,
                                                          const u64* __restrict__ word_off, uint32_t* __restrict__ words) {
    const uint32_t lane = threadIdx.x & 63;
    const u64 r = (u64)blockIdx.x * (SAM_BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= rd.R) return;
    const uint32_t s = rd.start[r];
    const u64 o = rd.base_off[r];
    const uint32_t len = (uint32_t)(rd.base_off[r + 1] - o);
    u64 at = words ? word_off[r] : 0;
    uint32_t n = 0;
    for (uint32_t j0 = 0; j0 < len; j0 += 64) {
        const uint32_t j = j0 + lane;
        bool differs = false;
        uint32_t k = 0, ref_ch = 0, site = 0;
        if (j < len) {
            site = s + j;
            const uint32_t c = min((uint32_t)rd.base[o + j], SAM_CODE_GAP);
            k = keep[(u64)site * 6 + c];
            ref_ch = rd.ref[site];
            differs = code_char(k) != ref_ch;
        }
        const u64 m = __ballot(differs);
        if (words && differs) {
            const uint32_t before = __popcll(m & ((1ull << lane) - 1));
            words[at + before] = pack_word(site + 1, char_mask(ref_ch), code_mask(k), k == SAM_CODE_N);
        }
        const uint32_t found = __popcll(m);
        at += found;
        n += found;
    }
    if (!words && lane == 0) n_words[r] = n;
}

// ---- order -----------------------------------------------------------------------------------------------------------
// Two corrected reads of the same (start, length) differ only where one of them has a word; the first such column
// decides, in ASCII order, with the reference character standing in for the read that has no word there.
struct SamLess {
    SamSortArgs a;
    __host__ __device__ int words_cmp(uint32_t x, uint32_t y) const {
        u64 i = a.word_off[x], j = a.word_off[y];
        const u64 ie = a.word_off[x + 1], je = a.word_off[y + 1];
        while (i < ie || j < je) {
            const uint32_t wx = i < ie ? a.words[i] : 0xFFFFFFFFu, wy = j < je ? a.words[j] : 0xFFFFFFFFu;
            const uint32_t px = i < ie ? (wx & 0xFFFFFu) : 0xFFFFFFFFu, py = j < je ? (wy & 0xFFFFFu) : 0xFFFFFFFFu;
            uint32_t cx, cy;
            if (px == py) {
                if (wx == wy) { i++; j++; continue; }
                cx = mask_char_h((wx >> 24) & 15); cy = mask_char_h((wy >> 24) & 15);
            } else if (px < py) {
                cx = mask_char_h((wx >> 24) & 15); cy = a.ref[px - 1];
            } else {
                cx = a.ref[py - 1]; cy = mask_char_h((wy >> 24) & 15);
            }
            return cx < cy ? -1 : 1;
        }
        return 0;
    }
    static __host__ __device__ uint32_t mask_char_h(uint32_t m) { return m == 1 ? 'A' : m == 2 ? 'C' : m == 4 ? 'G' : m == 8 ? 'T' : 'N'; }
    __host__ __device__ bool operator()(uint32_t x, uint32_t y) const {
        if (x == y) return false;
        const uint32_t sx = a.start[x], sy = a.start[y];
        if (sx != sy) return sx < sy;
        const u64 lx = a.base_off[x + 1] - a.base_off[x], ly = a.base_off[y + 1] - a.base_off[y];
        if (lx != ly) return lx < ly;
        const int c = words_cmp(x, y);
        return c ? c < 0 : x < y;
    }
};

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_iota(uint32_t R, uint32_t* __restrict__ v) {
    const u64 i = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (i < R) v[i] = (uint32_t)i;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_heads(SamSortArgs a, uint32_t R, const uint32_t* __restrict__ order, uint32_t* __restrict__ head) {
    const u64 s = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (s >= R) return;
    uint32_t h = 1;
    if (s > 0) {
        const uint32_t x = order[s - 1], y = order[s];
        const bool same_window = a.start[x] == a.start[y] && a.base_off[x + 1] - a.base_off[x] == a.base_off[y + 1] - a.base_off[y];
        if (same_window) {
            u64 i = a.word_off[x], j = a.word_off[y];
            const u64 ie = a.word_off[x + 1], je = a.word_off[y + 1];
            bool same = ie - i == je - j;
            for (; same && i < ie; i++, j++) same = a.words[i] == a.words[j];
            h = same ? 0 : 1;
        }
    }
    head[s] = h;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_groups(uint32_t R, const uint32_t* __restrict__ order, const uint32_t* __restrict__ head,
                                                           const u64* __restrict__ head_off, const u64* __restrict__ word_off,
                                                           uint32_t* __restrict__ group_off, uint32_t* __restrict__ lead_words) {
    const u64 s = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (s > R) return;
    if (s == R) { group_off[head_off[R]] = R; return; }
    if (!head[s]) return;
    const u64 g = head_off[s];
    const uint32_t x = order[s];
    group_off[g] = (uint32_t)s;
    lead_words[g] = (uint32_t)(word_off[x + 1] - word_off[x]);
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_merge(SamSortArgs a, uint32_t n_merged, const uint32_t* __restrict__ order,
                                                          const uint32_t* __restrict__ group_off, const u64* __restrict__ merged_off, SamMergedDev out) {
    const uint32_t lane = threadIdx.x & 63;
    const u64 g = (u64)blockIdx.x * (SAM_BLOCK / 64) + (threadIdx.x >> 6);
    if (g >= n_merged) return;
    const uint32_t lo = group_off[g], x = order[lo];
    const u64 from = a.word_off[x], n = a.word_off[x + 1] - from, to = merged_off[g];
    for (u64 i = lane; i < n; i += 64) out.read_word[to + i] = a.words[from + i];
    if (lane == 0) {
        const uint32_t s = a.start[x], len = (uint32_t)(a.base_off[x + 1] - a.base_off[x]);
        out.read_off[g] = (uint32_t)to;
        if (g + 1 == n_merged) out.read_off[n_merged] = (uint32_t)(to + n);
        out.start[g] = (int32_t)(s + 1);
        out.end[g] = (int32_t)(s + len);
        out.degree[g] = (int32_t)(group_off[g + 1] - lo);
    }
}

inline unsigned blocks_for(u64 n, uint32_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

hipError_t launch_sam_pileup(const SamReadsDev& rd, uint32_t* freq, uint32_t* bad_base, hipStream_t stream) {
    if (rd.R == 0 || rd.G == 0) return hipSuccess;
    const uint32_t tiles = (rd.G + SAM_TILE - 1) / SAM_TILE;
    const uint32_t want_chunks = SAM_PILE_WGS / tiles ? SAM_PILE_WGS / tiles : 1;
    uint32_t per = (uint32_t)(((u64)rd.R + want_chunks - 1) / want_chunks);
    per = (std::max(per, SAM_BLOCK) + SAM_BLOCK - 1) / SAM_BLOCK * SAM_BLOCK;
    const uint32_t chunks = (uint32_t)(((u64)rd.R + per - 1) / per);
    hipLaunchKernelGGL(k_sam_pileup, dim3(tiles, chunks), dim3(SAM_BLOCK), 0, stream, rd, per, freq, bad_base);
    return hipGetLastError();
}

hipError_t launch_sam_keep(const uint32_t* freq, uint32_t G, double min_af, uint32_t min_depth, uint8_t* keep, hipStream_t stream) {
    if (G == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sam_keep, dim3(blocks_for(G, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, freq, G, min_af, min_depth, keep);
    return hipGetLastError();
}

hipError_t launch_sam_count(const SamReadsDev& rd, const uint8_t* keep, uint32_t* n_words, hipStream_t stream) {
    if (rd.R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sam_words, dim3(blocks_for(rd.R, SAM_BLOCK / 64)), dim3(SAM_BLOCK), 0, stream, rd, keep, n_words,
                       (const u64*)nullptr, (uint32_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_sam_words(const SamReadsDev& rd, const uint8_t* keep, const unsigned long long* word_off, uint32_t* words, hipStream_t stream) {
    if (rd.R == 0 || !words) return hipSuccess;
    hipLaunchKernelGGL(k_sam_words, dim3(blocks_for(rd.R, SAM_BLOCK / 64)), dim3(SAM_BLOCK), 0, stream, rd, keep, (uint32_t*)nullptr, word_off, words);
    return hipGetLastError();
}

// (the input holds n + 1 entries too; the last one does not enter any sum)
hipError_t sam_scan_temp_bytes(uint32_t n, size_t* bytes) {
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const uint32_t*)nullptr, (u64*)nullptr, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), nullptr);
}
hipError_t launch_sam_scan(const uint32_t* in, unsigned long long* out, uint32_t n, void* temp, size_t temp_bytes, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, temp_bytes, in, out, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), stream);
}

hipError_t sam_sort_temp_bytes(uint32_t R, size_t* bytes) {
    *bytes = 0;
    return rocprim::merge_sort(nullptr, *bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)R, SamLess{}, nullptr);
}
hipError_t launch_sam_sort(const SamSortArgs& a, uint32_t R, uint32_t* iota, uint32_t* order, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sam_iota, dim3(blocks_for(R, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, R, iota);
    if (hipError_t e = hipGetLastError()) return e;
    return rocprim::merge_sort(temp, temp_bytes, iota, order, (size_t)R, SamLess{a}, stream);
}

hipError_t launch_sam_heads(const SamSortArgs& a, uint32_t R, const uint32_t* order, uint32_t* head, hipStream_t stream) {
    if (R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sam_heads, dim3(blocks_for(R, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, a, R, order, head);
    return hipGetLastError();
}

hipError_t launch_sam_groups(uint32_t R, const uint32_t* order, const uint32_t* head, const unsigned long long* head_off,
                             const unsigned long long* word_off, uint32_t* group_off, uint32_t* lead_words, hipStream_t stream) {
    if (R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sam_groups, dim3(blocks_for((u64)R + 1, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, R, order, head, head_off, word_off,
                       group_off, lead_words);
    return hipGetLastError();
}

hipError_t launch_sam_merge(const SamSortArgs& a, uint32_t n_merged, const uint32_t* order, const uint32_t* group_off,
                            const unsigned long long* merged_off, const SamMergedDev& out, hipStream_t stream) {
    if (n_merged == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sam_merge, dim3(blocks_for(n_merged, SAM_BLOCK / 64)), dim3(SAM_BLOCK), 0, stream, a, n_merged, order, group_off,
                       merged_off, out);
    return hipGetLastError();
}

}  // namespace wepp
