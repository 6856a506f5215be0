// resolve_kernels.hip -- wepp_epp_resolve: which reads carry each residual mutation, and which selected haplotype
// their nearest ones point to (arena::resolve_unaccounted_mutations, src/WEPP/arena.cpp:739-892).
//
// Mark: one thread per read walks its entries against the residual mutations inside its window (the list is
// sorted by position, stably; positions do not interact, so the caller's order only matters within one).  A
// count pass, scans and a write pass give the touched reads r' as a compact read batch and the (mutation,
// read) relations read-major; a stable sort by mutation makes them mutation-major with the reads ascending.
// Assign: k_assign (assign_kernels.hip) on the touched reads, tie masks kept.
// Tally: a workgroup per (mutation, chunk of its relations); a lane owns the 4 columns of a 256-haplotype slab
// it owns in k_assign and reads the tie masks as they were written.  Everything is integer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "resolve.hpp"

namespace wepp {

namespace {

constexpr uint32_t N_WORD_BITS = (15u << 24) | (1u << 28);   // mut_nuc 15, is_missing

// first i in [0, n) with v[i] >= x
template <typename I>
__device__ __forceinline__ I lower_bound_u32(const uint32_t* __restrict__ v, I n, uint32_t x) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = lo + (hi - lo) / 2;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The three-way rule of arena.cpp:759-791 for read r.  n_rel / n_words receive the relations and the entries
// of r'; with WRITE they are stored from rel_at / word_at on.
template <bool WRITE>
__device__ __forceinline__ void mark_read(const MarkArgs& a, uint32_t r, unsigned long long rel_at,
                                          unsigned long long word_at, uint32_t& n_rel, uint32_t& n_words) {
    const uint32_t off0 = a.read_off[r], n = a.read_off[r + 1] - off0;
    const uint32_t st = (uint32_t)a.start[r], en = (uint32_t)a.end[r];
    uint32_t i = lower_bound_u32(a.res_pos, a.M, st);
    uint32_t j = 0, nr = 0, nw = 0;
    auto emit = [&](uint32_t w) {
        if (WRITE) a.out_word[word_at + nw] = w;
        nw++;
    };
    while (i < a.M) {
        const uint32_t p = a.res_pos[i];
        if (p > en) break;
        while (j < n) {
            const uint32_t w = a.read_word[off0 + j];
            if ((w & 0xFFFFFu) >= p) break;
            emit(w);
            j++;
        }
        const bool have = j < n && (a.read_word[off0 + j] & 0xFFFFFu) == p;
        uint32_t cur = have ? a.read_word[off0 + j] : 0u;          // r' at p; 0: no entry (a word is never 0)
        for (; i < a.M && a.res_pos[i] == p; i++) {
            const uint32_t rw = a.res_word[i], rref = (rw >> 20) & 15u, rmut = (rw >> 24) & 15u;
            uint32_t rel = 0;                                       // 1 covered, 2 masked
            if (cur) {
                const uint32_t cm = (cur >> 24) & 15u;
                if (cm == 15u) rel = 2;
                else if (cm == rmut) { cur |= N_WORD_BITS; rel = 1; }
            } else if (rmut == rref) {
                cur = p | (rref << 20) | N_WORD_BITS;
                rel = 1;
            }
            if (rel) {
                if (WRITE) {
                    const uint32_t m = a.res_idx[i];
                    a.rel_key[rel_at + nr] = m;
                    a.rel_val[rel_at + nr] = r | (rel == 2 ? RES_MASKED : 0u);
                    atomicAdd(rel == 2 ? &a.n_masked[m] : &a.n_covered[m], 1u);
                }
                nr++;
            }
        }
        if (cur) emit(cur);
        if (have) j++;
    }
    for (; j < n; j++) emit(a.read_word[off0 + j]);
    n_rel = nr;
    n_words = nw;
}

__global__ void k_resolve_count(MarkArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.R) return;
    const uint32_t r = a.order[s];
    uint32_t nr, nw;
    mark_read<false>(a, r, 0, 0, nr, nw);
    const uint32_t t = nr ? 1u : 0u;
    a.n_rel[r] = nr;
    a.n_words[r] = t ? nw : 0u;
    a.touched[r] = t;
    a.touched_place[s] = t;
}

__global__ void k_resolve_write(MarkArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.R) return;
    if (s == 0) a.out_off[a.compact[a.R]] = (uint32_t)a.word_at[a.R];
    const uint32_t r = a.order[s];
    if (!a.touched[r]) return;
    const uint32_t t = (uint32_t)a.compact[r];
    const unsigned long long wa = a.word_at[r];
    a.out_off[t] = (uint32_t)wa;
    a.out_start[t] = a.start[r];
    a.out_end[t] = a.end[r];
    a.out_degree[t] = a.degree[r];
    // the touched reads keep their relative index order: their (start, end, index) order is the old one, thinned
    a.out_order[a.place_at[s]] = t;
    uint32_t nr, nw;
    mark_read<true>(a, r, a.rel_at[r], wa, nr, nw);
}

__global__ void k_resolve_offsets(const uint32_t* __restrict__ keys, unsigned long long n, uint32_t M,
                                  unsigned long long* __restrict__ rel_off) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > M) return;
    rel_off[m] = m == M ? n : lower_bound_u32(keys, n, m);
}

// A workgroup takes the chunks blockIdx.y, blockIdx.y + gridDim.y, .. of mutation blockIdx.x; its waves take
// every RES_WAVES-th relation of a chunk.  One slab at a time: 4 counts and 4 sums per lane in registers, the
// waves' partial results meet in LDS, a thread per column adds them up.
__global__ __launch_bounds__(64 * RES_WAVES) void k_resolve_tally(TallyArgs a) {
    __shared__ uint32_t l_cnt[RES_WAVES][ASG_SLAB];
    __shared__ unsigned long long l_deg[RES_WAVES][ASG_SLAB];
    const uint32_t m = blockIdx.x;
    const unsigned long long b = a.rel_off[m], e = a.rel_off[m + 1];
    const unsigned long long nchunks = (e - b + RES_CHUNK - 1) / RES_CHUNK;
    if (blockIdx.y >= nchunks) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nslabs = a.Kp / ASG_SLAB;
    for (uint32_t slab = 0; slab < nslabs; slab++) {
        uint32_t cnt[ASG_LANE_HAPS] = {0, 0, 0, 0};
        unsigned long long deg[ASG_LANE_HAPS] = {0, 0, 0, 0};
        for (unsigned long long c = blockIdx.y; c < nchunks; c += gridDim.y) {
            const unsigned long long i0 = b + c * RES_CHUNK, i1 = min(e, i0 + RES_CHUNK);
            for (unsigned long long i = i0 + wave; i < i1; i += RES_WAVES) {
                const uint32_t t = (uint32_t)a.compact[a.rel_read[i] & ~RES_MASKED];
                const unsigned long long d = (unsigned long long)(uint32_t)a.degree[t];
                const unsigned long long* tm = a.ties + ((size_t)t * nslabs + slab) * ASG_LANE_HAPS;
#pragma unroll
                for (uint32_t j = 0; j < ASG_LANE_HAPS; j++) {
                    const uint32_t bit = (uint32_t)(tm[j] >> lane) & 1u;
                    cnt[j] += bit;
                    deg[j] += bit ? d : 0ull;
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < ASG_LANE_HAPS; j++) {
            l_cnt[wave][lane * ASG_LANE_HAPS + j] = cnt[j];
            l_deg[wave][lane * ASG_LANE_HAPS + j] = deg[j];
        }
        __syncthreads();
        {
            uint32_t c = 0;
            unsigned long long d = 0;
#pragma unroll
            for (uint32_t w = 0; w < RES_WAVES; w++) { c += l_cnt[w][threadIdx.x]; d += l_deg[w][threadIdx.x]; }
            const uint32_t k = slab * ASG_SLAB + threadIdx.x;
            if (k < a.K && c) {
                const size_t at = (size_t)m * a.K + k;
                if (nchunks == 1) {              // the only writer of this row
                    a.hap_reads[at] = c;
                    a.hap_degree[at] = d;
                } else {
                    atomicAdd(&a.hap_reads[at], c);
                    if (d) atomicAdd(&a.hap_degree[at], d);
                }
            }
        }
        __syncthreads();
    }
}

// a wave per mutation: the maximum over the columns that appeared, then the columns attaining it, 64 per ballot
__global__ void k_resolve_best(const uint32_t* __restrict__ hap_reads, const unsigned long long* __restrict__ hap_degree,
                               uint32_t M, uint32_t K, long long* __restrict__ best_degree, uint32_t* __restrict__ best_mask) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (m >= M) return;
    const uint32_t KW = (K + 31) / 32;
    const uint32_t* hr = hap_reads + (size_t)m * K;
    const unsigned long long* hd = hap_degree + (size_t)m * K;
    long long best = 0;
    for (uint32_t k0 = 0; k0 < K; k0 += 64) {
        const uint32_t k = k0 + lane;
        if (k < K && hr[k]) best = max(best, (long long)hd[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
    for (uint32_t k0 = 0; k0 < K; k0 += 64) {
        const uint32_t k = k0 + lane;
        const unsigned long long bal = __ballot(k < K && hr[k] && (long long)hd[k] == best);
        if (lane == 0) {
            best_mask[(size_t)m * KW + k0 / 32] = (uint32_t)bal;
            if (k0 / 32 + 1 < KW) best_mask[(size_t)m * KW + k0 / 32 + 1] = (uint32_t)(bal >> 32);
        }
    }
    if (lane == 0) best_degree[m] = best;
}

}  // namespace

hipError_t launch_resolve_count(const MarkArgs& a, hipStream_t stream) {
    if (a.R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_resolve_count, dim3((a.R + 255) / 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_resolve_write(const MarkArgs& a, hipStream_t stream) {
    if (a.R == 0) return hipSuccess;
    hipLaunchKernelGGL(k_resolve_write, dim3((a.R + 255) / 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t resolve_sort_temp_bytes(uint64_t n, uint32_t key_bits, size_t* bytes) {
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                     (uint32_t*)nullptr, n, 0, key_bits, nullptr);
}

hipError_t launch_resolve_sort(const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                               uint64_t n, uint32_t key_bits, void* temp, size_t temp_bytes, hipStream_t stream) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, key_bits, stream);
}

hipError_t launch_resolve_offsets(const uint32_t* keys, uint64_t n, uint32_t M, unsigned long long* rel_off, hipStream_t stream) {
    hipLaunchKernelGGL(k_resolve_offsets, dim3(M / 256 + 1), dim3(256), 0, stream, keys, (unsigned long long)n, M, rel_off);
    return hipGetLastError();
}

hipError_t launch_resolve_tally(const TallyArgs& a, uint64_t max_chunks, hipStream_t stream) {
    if (a.M == 0 || max_chunks == 0) return hipSuccess;
    const uint32_t wgs = (uint32_t)std::min<uint64_t>(RES_MAX_CHUNK_WGS, max_chunks);
    hipLaunchKernelGGL(k_resolve_tally, dim3(a.M, wgs), dim3(64 * RES_WAVES), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_resolve_best(const uint32_t* hap_reads, const unsigned long long* hap_degree, uint32_t M, uint32_t K,
                               long long* best_degree, uint32_t* best_mask, hipStream_t stream) {
    if (M == 0) return hipSuccess;
    hipLaunchKernelGGL(k_resolve_best, dim3((M + 3) / 4), dim3(256), 0, stream, hap_reads, hap_degree, M, K, best_degree, best_mask);
    return hipGetLastError();
}

}  // namespace wepp
