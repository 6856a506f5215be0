// sam_subsample_kernels.hip -- the device side of wepp_sam_build_subsampled (sam_subsample.hpp; host side
// sam_subsample_capi.cpp): the thresholds of all trials by a radix select over keys that are computed where they are
// needed, the trial pile-up of a batch of trials per workgroup, the divergence of every trial's table from the full
// table in a fixed order of summation, the pick and the compaction of the kept reads.  Integers throughout, except the
// fp64 divergence.  No key and no permutation is ever stored: membership of read r in trial t is
// sub_hash(trial_hash[t] ^ r) <= thr[t].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sam_subsample.hpp"

namespace wepp {
namespace {

using u64 = unsigned long long;

__device__ __forceinline__ u64 shfl64(u64 v, int lane) {
    const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// ---- thresholds -------------------------------------------------------------------------------------------------------
// Workgroup (k, t) histograms one digit of the keys of chunk k of the reads under trial t in LDS and adds its non-zero
// bins to the trial's histogram.  In the first pass every key takes part; later only the few under the prefix do.
__global__ __launch_bounds__(SAM_BLOCK) void k_sub_histogram(const u64* __restrict__ trial_hash, const u64* __restrict__ prefix, uint32_t n_reads,
                                                              uint32_t reads_per_chunk, uint32_t shift, uint32_t width, int first,
                                                              uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[SUB_BINS];
    const uint32_t tid = threadIdx.x, t = blockIdx.y;
    for (uint32_t i = tid; i < SUB_BINS; i += SAM_BLOCK) bins[i] = 0;
    __syncthreads();
    const u64 h = trial_hash[t], want = first ? 0 : prefix[t];
    const uint32_t above = shift + width, digit_mask = (1u << width) - 1;
    const u64 r0 = (u64)blockIdx.x * reads_per_chunk, r1 = min((u64)n_reads, r0 + reads_per_chunk);
    for (u64 r = r0 + tid; r < r1; r += SAM_BLOCK) {
        const u64 key = sub_hash(h ^ r);
        if (first || (key >> above) == want) atomicAdd(&bins[(uint32_t)(key >> shift) & digit_mask], 1u);
    }
    __syncthreads();
    for (uint32_t i = tid; i < SUB_BINS; i += SAM_BLOCK) {
        const uint32_t v = bins[i];
        if (v) atomicAdd(&hist[(u64)t * SUB_BINS + i], v);
    }
}

// one wave per trial: the bins' running sum in lane order, 64 bins a round
__global__ __launch_bounds__(SAM_BLOCK) void k_sub_pick_digit(const uint32_t* __restrict__ hist, uint32_t n_trials, uint32_t width,
                                                               u64* __restrict__ prefix, uint32_t* __restrict__ rank) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t t = blockIdx.x * (SAM_BLOCK / 64) + (threadIdx.x >> 6);
    if (t >= n_trials) return;
    const uint32_t want = rank[t], n_bins = 1u << width;
    uint32_t before = 0;                                   // keys in the bins of earlier rounds
    for (uint32_t b0 = 0; b0 < n_bins; b0 += 64) {
        const uint32_t v = hist[(u64)t * SUB_BINS + b0 + lane];   // (width >= 6: a round never leaves the digit's bins)
        uint32_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if ((int)lane >= d) incl += up;
        }
        const bool here = before + incl - v <= want && want < before + incl;
        const u64 found = __ballot(here);
        if (found) {                                       // (the bins' counts are positive where `here` holds: one lane)
            if (here) {
                prefix[t] = (prefix[t] << width) | (u64)(b0 + lane);
                rank[t] = want - (before + incl - v);
            }
            return;
        }
        before += __shfl(incl, 63);
    }
}

// ---- the tiles' read lists ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAM_BLOCK) void k_sub_bin(SamReadsDev rd, const u64* __restrict__ tile_off, uint32_t* __restrict__ counter,
                                                        uint32_t* __restrict__ list) {
    const u64 r = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (r >= rd.R) return;
    const uint32_t s = rd.start[r], len = (uint32_t)(rd.base_off[r + 1] - rd.base_off[r]);
    if (len == 0) return;
    for (uint32_t tile = s / SUB_TILE; tile <= (s + len - 1) / SUB_TILE; tile++) {
        const uint32_t at = atomicAdd(&counter[tile], 1u);
        if (list) list[tile_off[tile] + at] = (uint32_t)r;
    }
}

// ---- trial pile-up ----------------------------------------------------------------------------------------------------
// Workgroup (tile, k, b) owns tile `tile` of SUB_TILE sites, chunk k of the tile's read list and the batch of SUB_BATCH
// trials b.  A lane takes one read of the list and finds the trials of the batch that hold it (one hash per trial);
// the wave then takes the reads that some trial holds one at a time, a lane per column as k_sam_pileup does, reads
// every column once and adds it to the counters of every trial the read belongs to.  32-bit counters: exact for any
// depth below 2^32 (a call holds fewer than 2^31 reads).
__global__ __launch_bounds__(SUB_PILE_BLOCK) void k_sub_pileup(SamReadsDev rd, const u64* __restrict__ tile_off, const uint32_t* __restrict__ list,
                                                           uint32_t per_chunk, const u64* __restrict__ trial_hash, const u64* __restrict__ thr,
                                                           uint32_t t0, uint32_t n_trials, uint32_t* __restrict__ tables) {
    __shared__ uint32_t cnt[SUB_BATCH * SUB_TILE * 6];
    const u64 list_end = tile_off[blockIdx.x + 1];
    const u64 l0 = tile_off[blockIdx.x] + (u64)blockIdx.y * per_chunk, l1 = min(list_end, l0 + per_chunk);
    if (l0 >= list_end) return;                            // (the whole workgroup: the grid is sized by the longest list)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b0 = blockIdx.z * SUB_BATCH, nb = min(SUB_BATCH, n_trials - b0);
    for (uint32_t i = tid; i < SUB_BATCH * SUB_TILE * 6; i += SUB_PILE_BLOCK) cnt[i] = 0;
    u64 h[SUB_BATCH], cut[SUB_BATCH];
#pragma unroll
    for (uint32_t b = 0; b < SUB_BATCH; b++) {
        const uint32_t t = t0 + b0 + min(b, nb - 1);
        h[b] = trial_hash[t]; cut[b] = thr[t];
    }
    __syncthreads();
    const uint32_t tile_lo = blockIdx.x * SUB_TILE, tile_hi = min(rd.G, tile_lo + SUB_TILE);
    for (u64 lb = l0 + wave * 64; lb < l1; lb += SUB_PILE_BLOCK) {
        const u64 i = lb + lane;
        uint32_t s = 0, len = 0, member = 0;
        u64 o = 0;
        if (i < l1) {
            const uint32_t r = list[i];
            s = rd.start[r]; o = rd.base_off[r]; len = (uint32_t)(rd.base_off[r + 1] - o);
#pragma unroll
            for (uint32_t b = 0; b < SUB_BATCH; b++)
                if (b < nb && sub_hash(h[b] ^ (u64)r) <= cut[b]) member |= 1u << b;
        }
        // A read's part inside the tile is at most SUB_TILE = 4 x 64 columns: four loads per lane hold it.  The loads of
        // the next read are issued before the counters of the current one are updated, so their latency lies behind
        // the LDS atomics and not in front of them.
        u64 live = __ballot(member != 0);
        uint32_t col[SUB_SEGMENTS], first = 0, in = 0;    // the current read: its bytes (0xFF outside), lane 0's site in the tile, its trials
        bool have = false;
        while (live || have) {
            uint32_t next_col[SUB_SEGMENTS], next_first = 0, next_in = 0;
#pragma unroll
            for (uint32_t k = 0; k < SUB_SEGMENTS; k++) next_col[k] = 0xFFu;
            const bool have_next = live != 0;
            if (have_next) {
                const int l = __ffsll((long long)live) - 1;
                live &= live - 1;
                const uint32_t rs = __shfl(s, l), rlen = __shfl(len, l);
                const u64 ro = shfl64(o, l);
                next_in = __shfl(member, l);
                const uint32_t lo = max(rs, tile_lo), hi = min(rs + rlen, tile_hi);
                next_first = lo - tile_lo;
#pragma unroll
                for (uint32_t k = 0; k < SUB_SEGMENTS; k++) {
                    const uint32_t p = lo + k * 64 + lane;
                    next_col[k] = p < hi ? (uint32_t)rd.base[ro + (p - rs)] : 0xFFu;
                }
            }
            if (have) {
#pragma unroll
                for (uint32_t k = 0; k < SUB_SEGMENTS; k++) {
                    const uint32_t c = col[k];
                    if (c > SAM_CODE_GAP) continue;        // (outside the read; a byte > 5 the full pile-up has reported: the call fails before this runs)
                    const uint32_t cell = (first + k * 64 + lane) * 6 + c;
                    for (uint32_t m = in; m; m &= m - 1) atomicAdd(&cnt[(__ffs((int)m) - 1) * (SUB_TILE * 6) + cell], 1u);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < SUB_SEGMENTS; k++) col[k] = next_col[k];
            first = next_first; in = next_in; have = have_next;
        }
    }
    __syncthreads();
    const uint32_t cells = (tile_hi - tile_lo) * 6;
    const u64 table = (u64)rd.G * 6;
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t i = tid; i < cells; i += SUB_PILE_BLOCK) {
            const uint32_t v = cnt[b * (SUB_TILE * 6) + i];
            if (v) atomicAdd(&tables[(b0 + b) * table + (u64)tile_lo * 6 + i], v);
        }
}

// ---- divergence -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAM_BLOCK) void k_sub_covered(const uint32_t* __restrict__ freq, uint32_t G, uint32_t* __restrict__ covered) {
    const uint32_t site = blockIdx.x * SAM_BLOCK + threadIdx.x;
    bool any = false;
    if (site < G)
        for (int c = 0; c < 6; c++) any |= freq[(u64)site * 6 + c] != 0;
    const uint32_t n = __popcll(__ballot(any));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(covered, n);
}

// One workgroup per trial.  Thread i sums the terms of the sites i, i + 256, ... in that order, cell by cell; the 256
// partial sums meet in a tree of fixed shape: the result is a function of the two tables alone.  Every operation is the
// IEEE double operation the rule writes down (no contraction into fused multiply-adds).
__global__ __launch_bounds__(SAM_BLOCK) void k_sub_divergence(const uint32_t* __restrict__ freq, const uint32_t* __restrict__ covered, uint32_t G,
                                                               const uint32_t* __restrict__ tables, uint32_t t0, double* __restrict__ divergence) {
#pragma clang fp contract(off)
    __shared__ uint32_t sites_seen;
    __shared__ double part[SAM_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint32_t* A = tables + (u64)blockIdx.x * G * 6;
    if (tid == 0) sites_seen = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t site = tid; site < G; site += SAM_BLOCK) {
        bool any = false;
        for (int c = 0; c < 6; c++) any |= A[(u64)site * 6 + c] != 0;
        mine += any;
    }
    if (mine) atomicAdd(&sites_seen, mine);
    __syncthreads();
    const double C = (double)*covered, Ct = (double)sites_seen;
    double acc = 0.0;
    for (uint32_t site = tid; site < G; site += SAM_BLOCK) {
        uint32_t f[6], a[6];
        u64 S = 0, At = 0;
        for (int c = 0; c < 6; c++) { f[c] = freq[(u64)site * 6 + c]; a[c] = A[(u64)site * 6 + c]; S += f[c]; At += a[c]; }
        if (S == 0) continue;
        const double dS = (double)S * C, dA = (double)At * Ct;
        for (int c = 0; c < 6; c++) {
            if (f[c] == 0) continue;
            const double p = (double)f[c] / dS;
            const double q = At ? (double)a[c] / dA : 0.0;
            const double term = p * (log(p) - log(fmax(q, 1e-10)));
            acc = acc + term;
        }
    }
    part[tid] = acc;
    __syncthreads();
    for (uint32_t s = SAM_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] = part[tid] + part[tid + s];
        __syncthreads();
    }
    if (tid == 0) divergence[t0 + blockIdx.x] = part[0];
}

// one workgroup: the smallest divergence, the lowest trial among equals
__global__ __launch_bounds__(SAM_BLOCK) void k_sub_argmin(const double* __restrict__ divergence, uint32_t n_trials, uint32_t* __restrict__ best) {
    __shared__ double val[SAM_BLOCK];
    __shared__ uint32_t idx[SAM_BLOCK];
    const uint32_t tid = threadIdx.x;
    double v = 0.0;
    uint32_t at = 0xFFFFFFFFu;
    for (uint32_t t = tid; t < n_trials; t += SAM_BLOCK) {
        const double d = divergence[t];
        if (at == 0xFFFFFFFFu || d < v) { v = d; at = t; }
    }
    val[tid] = v; idx[tid] = at;
    __syncthreads();
    for (uint32_t s = SAM_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s && idx[tid + s] != 0xFFFFFFFFu) {
            const bool better = idx[tid] == 0xFFFFFFFFu || val[tid + s] < val[tid] || (val[tid + s] == val[tid] && idx[tid + s] < idx[tid]);
            if (better) { val[tid] = val[tid + s]; idx[tid] = idx[tid + s]; }
        }
        __syncthreads();
    }
    if (tid == 0) *best = idx[0];
}

// ---- compaction -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAM_BLOCK) void k_sub_flags(uint32_t R, const u64* __restrict__ trial_hash, const u64* __restrict__ thr,
                                                          const uint32_t* __restrict__ best, uint32_t* __restrict__ flag) {
    const u64 r = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (r >= R) return;
    const uint32_t t = *best;
    flag[r] = sub_hash(trial_hash[t] ^ r) <= thr[t] ? 1u : 0u;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sub_kept(SamReadsDev rd, const uint32_t* __restrict__ flag, const u64* __restrict__ flag_off,
                                                         uint32_t* __restrict__ kept, uint32_t* __restrict__ kept_start, uint32_t* __restrict__ kept_len) {
    const u64 r = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (r >= rd.R || !flag[r]) return;
    const u64 j = flag_off[r];
    kept[j] = (uint32_t)r;
    kept_start[j] = rd.start[r];
    kept_len[j] = (uint32_t)(rd.base_off[r + 1] - rd.base_off[r]);
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sub_gather(SamReadsDev rd, uint32_t n_kept, const uint32_t* __restrict__ kept,
                                                           const u64* __restrict__ kept_off, uint8_t* __restrict__ kept_base) {
    const uint32_t lane = threadIdx.x & 63;
    const u64 j = (u64)blockIdx.x * (SAM_BLOCK / 64) + (threadIdx.x >> 6);
    if (j >= n_kept) return;
    const uint32_t r = kept[j];
    const u64 from = rd.base_off[r], n = rd.base_off[r + 1] - from, to = kept_off[j];
    for (u64 i = lane; i < n; i += 64) kept_base[to + i] = rd.base[from + i];
}

inline unsigned blocks_for(u64 n, uint32_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

hipError_t launch_sub_histogram(const unsigned long long* trial_hash, const unsigned long long* prefix, uint32_t n_trials, uint32_t n_reads,
                                uint32_t shift, uint32_t width, bool first, uint32_t* hist, hipStream_t stream) {
    if (n_trials == 0 || n_reads == 0) return hipSuccess;
    // about 4096 workgroups a launch, none with fewer than 4096 reads unless the reads are fewer
    const uint32_t want_chunks = std::max(1u, 4096u / n_trials);
    uint32_t per = (uint32_t)(((u64)n_reads + want_chunks - 1) / want_chunks);
    per = (std::max(per, 4096u) + SAM_BLOCK - 1) / SAM_BLOCK * SAM_BLOCK;
    const uint32_t chunks = (uint32_t)(((u64)n_reads + per - 1) / per);
    hipLaunchKernelGGL(k_sub_histogram, dim3(chunks, n_trials), dim3(SAM_BLOCK), 0, stream, trial_hash, prefix, n_reads, per, shift, width,
                       first ? 1 : 0, hist);
    return hipGetLastError();
}

hipError_t launch_sub_pick_digit(const uint32_t* hist, uint32_t n_trials, uint32_t width, unsigned long long* prefix, uint32_t* rank, hipStream_t stream) {
    if (n_trials == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sub_pick_digit, dim3(blocks_for(n_trials, SAM_BLOCK / 64)), dim3(SAM_BLOCK), 0, stream, hist, n_trials, width, prefix, rank);
    return hipGetLastError();
}

hipError_t launch_sub_bin_count(const SamReadsDev& rd, uint32_t* tile_count, hipStream_t stream) {
    if (rd.R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sub_bin, dim3(blocks_for(rd.R, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, rd, (const u64*)nullptr, tile_count, (uint32_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_sub_bin_fill(const SamReadsDev& rd, const unsigned long long* tile_off, uint32_t* cursor, uint32_t* list, hipStream_t stream) {
    if (rd.R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sub_bin, dim3(blocks_for(rd.R, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, rd, tile_off, cursor, list);
    return hipGetLastError();
}

hipError_t launch_sub_pileup(const SamReadsDev& rd, const unsigned long long* tile_off, const uint32_t* list, uint32_t longest_list,
                             const unsigned long long* trial_hash, const unsigned long long* thr, uint32_t t0, uint32_t n_trials,
                             uint32_t* tables, hipStream_t stream) {
    if (rd.R == 0 || rd.G == 0 || n_trials == 0 || longest_list == 0) return hipSuccess;
    const uint32_t tiles = (rd.G + SUB_TILE - 1) / SUB_TILE, batches = (n_trials + SUB_BATCH - 1) / SUB_BATCH;
    const u64 fixed = (u64)tiles * batches;
    const uint32_t want_chunks = (uint32_t)std::max<u64>(1, SUB_PILE_WGS / fixed);
    uint32_t per = (longest_list + want_chunks - 1) / want_chunks;
    per = (std::max(per, SUB_CHUNK) + SUB_CHUNK - 1) / SUB_CHUNK * SUB_CHUNK;
    const uint32_t chunks = (longest_list + per - 1) / per;
    hipLaunchKernelGGL(k_sub_pileup, dim3(tiles, chunks, batches), dim3(SUB_PILE_BLOCK), 0, stream, rd, tile_off, list, per, trial_hash, thr, t0, n_trials,
                       tables);
    return hipGetLastError();
}

hipError_t launch_sub_covered(const uint32_t* freq, uint32_t G, uint32_t* covered, hipStream_t stream) {
    if (G == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sub_covered, dim3(blocks_for(G, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, freq, G, covered);
    return hipGetLastError();
}

hipError_t launch_sub_divergence(const uint32_t* freq, const uint32_t* covered, uint32_t G, const uint32_t* tables, uint32_t t0, uint32_t n_trials,
                                 double* divergence, hipStream_t stream) {
    if (n_trials == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sub_divergence, dim3(n_trials), dim3(SAM_BLOCK), 0, stream, freq, covered, G, tables, t0, divergence);
    return hipGetLastError();
}

hipError_t launch_sub_argmin(const double* divergence, uint32_t n_trials, uint32_t* best, hipStream_t stream) {
    hipLaunchKernelGGL(k_sub_argmin, dim3(1), dim3(SAM_BLOCK), 0, stream, divergence, n_trials, best);
    return hipGetLastError();
}

hipError_t launch_sub_flags(uint32_t R, const unsigned long long* trial_hash, const unsigned long long* thr, const uint32_t* best, uint32_t* flag,
                            hipStream_t stream) {
    if (R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sub_flags, dim3(blocks_for(R, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, R, trial_hash, thr, best, flag);
    return hipGetLastError();
}

hipError_t launch_sub_kept(const SamReadsDev& rd, const uint32_t* flag, const unsigned long long* flag_off, uint32_t* kept, uint32_t* kept_start,
                           uint32_t* kept_len, hipStream_t stream) {
    if (rd.R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sub_kept, dim3(blocks_for(rd.R, SAM_BLOCK)), dim3(SAM_BLOCK), 0, stream, rd, flag, flag_off, kept, kept_start, kept_len);
    return hipGetLastError();
}

hipError_t launch_sub_gather(const SamReadsDev& rd, uint32_t n_kept, const uint32_t* kept, const unsigned long long* kept_off, uint8_t* kept_base,
                             hipStream_t stream) {
    if (n_kept == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sub_gather, dim3(blocks_for(n_kept, SAM_BLOCK / 64)), dim3(SAM_BLOCK), 0, stream, rd, n_kept, kept, kept_off, kept_base);
    return hipGetLastError();
}

}  // namespace wepp
