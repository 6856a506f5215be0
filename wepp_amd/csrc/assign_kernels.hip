// assign_kernels.hip -- wepp_epp_assign: every read against a SELECTION of haplotypes
// (arena::dump_read2haplotype_mapping, src/WEPP/arena.cpp:590-696: reads x selected haplotypes calls of
// haplotype::mutation_distance, src/WEPP/haplotype.hpp:123-173).
//
// The selection's genotypes are laid out once per call as a position-major table: geno[p][k] = allele mask
// of haplotype sel[k] at p (0 = reference) and pre[p][k] = its non-reference positions <= p.  With them
//   d(r, k) = pre[end][k] - pre[start - 1][k] + #{entries of r that are not N}
//             - sum over the entries e of r inside [start, end] with geno[pos(e)][k] != 0 of
//               (1 + [e is not N and e.mut == geno[pos(e)][k]])
// (every position of the window where the haplotype differs from the reference costs one, every listed allele
// that is not N costs one, and where both meet the pair costs 0 -- N or equal alleles -- or 1).
// A wave takes one read; a lane owns 4 consecutive columns, so a row segment is one dword of geno and two of
// pre per lane, and the bytes are compared SWAR-style.  Everything is integer and order-independent.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "assign.hpp"

namespace wepp {

namespace {

constexpr uint32_t NIB = 0x0F0F0F0Fu, ONES = 0x01010101u;
// bytes hold values 0 .. 15: 1 in every byte that is not zero
__device__ __forceinline__ uint32_t nz_bytes(uint32_t v) { return ((v + NIB) >> 4) & ONES; }

// ---- the genotype table ----------------------------------------------------------------------------------
// one thread per column walks parent_dfs from its haplotype to the root.  The deepest mutation at a
// position wins: a cell is written once, by the first (deepest) node that names its position, and carries the
// marker bit 0x80 from then on (a back-mutation to the reference base leaves 0x80: claimed, reference).  A
// column belongs to one thread, so no cell is ever touched by two.
__global__ void k_assign_geno(const uint32_t* __restrict__ node_woff, const uint32_t* __restrict__ words,
                              const uint32_t* __restrict__ parent_dfs, const uint32_t* __restrict__ sel, uint32_t K,
                              uint32_t Kp, uint32_t max_pos, uint8_t* geno) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    uint32_t n = sel[k];
    for (;;) {
        const uint32_t w1 = node_woff[n + 1];
        for (uint32_t w = node_woff[n]; w < w1; w++) {
            const uint32_t word = words[w];
            const uint32_t p = word & 0xFFFFFu;
            if (p > max_pos) continue;
            uint8_t* cell = geno + (size_t)p * Kp + k;
            if (*cell == 0) {
                const uint32_t mut = (word >> 26) & 15u, ref = 1u << ((word >> 20) & 3u);
                *cell = (uint8_t)(0x80u | (mut == ref ? 0u : mut));
            }
        }
        if (n == 0) break;
        const uint32_t p = parent_dfs[n];
        if (p >= n) break;          // (pre-order: a parent precedes its children)
        n = p;
    }
}

// prefix counts down the columns as a blocked scan: (1) markers off + non-reference cells per block of
// ASG_SCAN_ROWS rows, (2) exclusive scan over the blocks of a column, (3) the rows of a block from its base.
// A thread owns 4 columns (one dword of a geno row, one 8-byte store of a pre row).
__global__ void k_assign_count(uint8_t* geno, uint32_t Kp, uint32_t rows, uint32_t* __restrict__ block_sums) {
    const uint32_t c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (c >= Kp) return;
    const uint32_t r0 = blockIdx.y * ASG_SCAN_ROWS, r1 = min(rows, r0 + ASG_SCAN_ROWS);
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint32_t r = r0; r < r1; r++) {
        uint32_t* cell = (uint32_t*)(geno + (size_t)r * Kp + c);
        const uint32_t v = *cell, g = v & NIB;
        if (v != g) *cell = g;
        const uint32_t nz = nz_bytes(g);
        s0 += nz & 1u; s1 += (nz >> 8) & 1u; s2 += (nz >> 16) & 1u; s3 += nz >> 24;
    }
    uint32_t* out = block_sums + (size_t)blockIdx.y * Kp + c;
    out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3;
}

__global__ void k_assign_blockscan(uint32_t* block_sums, uint32_t Kp, uint32_t nblk, uint32_t* overflow) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Kp) return;
    uint32_t run = 0;
    for (uint32_t b = 0; b < nblk; b++) {
        const uint32_t t = block_sums[(size_t)b * Kp + c];
        block_sums[(size_t)b * Kp + c] = run;
        run += t;
    }
    if (run > ASG_MAX_PRE) atomicMax(overflow, run);
}

__global__ void k_assign_pre(const uint8_t* __restrict__ geno, uint32_t Kp, uint32_t rows,
                             const uint32_t* __restrict__ block_sums, uint16_t* __restrict__ pre) {
    const uint32_t c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (c >= Kp) return;
    const uint32_t r0 = blockIdx.y * ASG_SCAN_ROWS, r1 = min(rows, r0 + ASG_SCAN_ROWS);
    const uint32_t* base = block_sums + (size_t)blockIdx.y * Kp + c;
    uint32_t s0 = base[0], s1 = base[1], s2 = base[2], s3 = base[3];
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t nz = nz_bytes(*(const uint32_t*)(geno + (size_t)r * Kp + c));
        s0 += nz & 1u; s1 += (nz >> 8) & 1u; s2 += (nz >> 16) & 1u; s3 += nz >> 24;
        const uint2 v = make_uint2((s0 & 0xFFFFu) | (s1 << 16), (s2 & 0xFFFFu) | (s3 << 16));
        *(uint2*)(pre + (size_t)r * Kp + c) = v;
    }
}

// ---- k_assign ----------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t wave_min(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

struct ReadView {                   // wave-uniform
    uint32_t off0, n;
    uint32_t st, en;
};

// distances of the lane's 4 columns in each of the ASG_REG_SLABS slabs of group g (INT32_MAX: no such column)
__device__ __forceinline__ void group_distances(const AssignArgs& a, const ReadView& rv, uint32_t g, uint32_t nslabs,
                                                uint32_t lane, int32_t (&d)[ASG_REG_SLABS * 4]) {
    const size_t rowE = (size_t)min(rv.en, a.max_pos) * a.Kp, rowS = (size_t)min(rv.st - 1, a.max_pos) * a.Kp;
    uint32_t acc[ASG_REG_SLABS];
    int32_t sub[ASG_REG_SLABS * 4];
#pragma unroll
    for (uint32_t q = 0; q < ASG_REG_SLABS; q++) {
        acc[q] = 0;
        const uint32_t slab = g * ASG_REG_SLABS + q;
        uint32_t lo = 0, hi = 0;
        if (slab < nslabs) {
            const uint32_t c = slab * ASG_SLAB + lane * ASG_LANE_HAPS;
            const uint2 pe = *(const uint2*)(a.pre + rowE + c), ps = *(const uint2*)(a.pre + rowS + c);
            // pre is monotone down a column: no field borrows from its neighbour
            lo = pe.x - ps.x;
            hi = pe.y - ps.y;
        }
        sub[q * 4 + 0] = -(int32_t)(lo & 0xFFFFu); sub[q * 4 + 1] = -(int32_t)(lo >> 16);
        sub[q * 4 + 2] = -(int32_t)(hi & 0xFFFFu); sub[q * 4 + 3] = -(int32_t)(hi >> 16);
    }
    auto flush = [&]() {
#pragma unroll
        for (uint32_t q = 0; q < ASG_REG_SLABS; q++) {
            sub[q * 4 + 0] += (int32_t)(acc[q] & 0xFFu); sub[q * 4 + 1] += (int32_t)((acc[q] >> 8) & 0xFFu);
            sub[q * 4 + 2] += (int32_t)((acc[q] >> 16) & 0xFFu); sub[q * 4 + 3] += (int32_t)(acc[q] >> 24);
            acc[q] = 0;
        }
    };
    uint32_t not_n = 0, pending = 0;
    for (uint32_t j = 0; j < rv.n; j++) {
        const uint32_t w = a.read_word[rv.off0 + j];
        const uint32_t pos = w & 0xFFFFFu, mut = (w >> 24) & 15u;
        const uint32_t real = mut != 15u;
        not_n += real;
        if (pos < rv.st || pos > rv.en || pos > a.max_pos) continue;
        const size_t row = (size_t)pos * a.Kp;
        const uint32_t mm = mut * ONES;
#pragma unroll
        for (uint32_t q = 0; q < ASG_REG_SLABS; q++) {
            const uint32_t slab = g * ASG_REG_SLABS + q;
            if (slab < nslabs) {
                const uint32_t g4 = *(const uint32_t*)(a.geno + row + slab * ASG_SLAB + lane * ASG_LANE_HAPS);
                const uint32_t nz = nz_bytes(g4), eq = ~((((g4 ^ mm) + NIB) >> 4)) & ONES;
                acc[q] += nz + (real ? eq : 0u);      // (eq implies nz: a listed allele is never 0)
            }
        }
        if (++pending == 127) { flush(); pending = 0; }   // a byte gains at most 2 per entry
    }
    flush();
#pragma unroll
    for (uint32_t q = 0; q < ASG_REG_SLABS; q++) {
        const uint32_t slab = g * ASG_REG_SLABS + q;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t col = slab * ASG_SLAB + lane * ASG_LANE_HAPS + j;
            d[q * 4 + j] = (slab < nslabs && col < a.K) ? (int32_t)not_n - sub[q * 4 + j] : INT32_MAX;
        }
    }
}

template <bool LDS_AGG>
__global__ __launch_bounds__(64 * ASG_WAVES) void k_assign(AssignArgs a) {
    HIP_DYNAMIC_SHARED(unsigned char, smem)
    unsigned long long* l_deg = (unsigned long long*)smem;        // [Kp]
    uint32_t* l_cnt = (uint32_t*)(l_deg + (LDS_AGG ? a.Kp : 0));  // [Kp]
    if (LDS_AGG) {
        for (uint32_t i = threadIdx.x; i < a.Kp; i += blockDim.x) { l_deg[i] = 0; l_cnt[i] = 0; }
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * ASG_WAVES;
    const uint32_t nslabs = a.Kp / ASG_SLAB, ngroups = (nslabs + ASG_REG_SLABS - 1) / ASG_REG_SLABS;
    // consecutive waves take consecutive reads of the (start, end) order: they ask for the same table rows
    for (uint32_t s = blockIdx.x * ASG_WAVES + wave; s < a.R; s += nwaves) {
        const uint32_t r = __builtin_amdgcn_readfirstlane(a.order[s]);
        ReadView rv;
        rv.off0 = __builtin_amdgcn_readfirstlane(a.read_off[r]);
        rv.n = __builtin_amdgcn_readfirstlane(a.read_off[r + 1]) - rv.off0;
        rv.st = (uint32_t)__builtin_amdgcn_readfirstlane(a.start[r]);
        rv.en = (uint32_t)__builtin_amdgcn_readfirstlane(a.end[r]);
        const uint32_t deg = (uint32_t)__builtin_amdgcn_readfirstlane(a.degree[r]);
        int32_t d[ASG_REG_SLABS * 4];
        int32_t best = INT32_MAX;
        for (uint32_t g = 0; g < ngroups; g++) {
            group_distances(a, rv, g, nslabs, lane, d);
#pragma unroll
            for (uint32_t i = 0; i < ASG_REG_SLABS * 4; i++) best = min(best, d[i]);
        }
        best = wave_min(best);
        // coverage: the window clipped to the genome, one bitmap word per lane and round
        const uint32_t cs = max(rv.st, 1u), ce = min(rv.en, a.genome_size);
        uint32_t ties = 0;
        for (uint32_t g = 0; g < ngroups; g++) {
            if (ngroups > 1) group_distances(a, rv, g, nslabs, lane, d);    // (one group: still in registers)
            unsigned long long ball[ASG_REG_SLABS * 4];
            unsigned long long any = 0;
#pragma unroll
            for (uint32_t q = 0; q < ASG_REG_SLABS; q++) {
                const uint32_t slab = g * ASG_REG_SLABS + q;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const bool tie = d[q * 4 + j] == best;
                    const unsigned long long b = __ballot(tie);
                    ball[q * 4 + j] = b;
                    any |= b;
                    ties += (uint32_t)__popcll(b);
                    if (slab < nslabs) {
                        if (a.ties && lane == j) a.ties[((size_t)r * nslabs + slab) * 4 + j] = b;
                        if (tie) {
                            const uint32_t col = slab * ASG_SLAB + lane * ASG_LANE_HAPS + j;
                            if (LDS_AGG) {
                                atomicAdd(&l_cnt[col], 1u);
                                if (deg) atomicAdd(&l_deg[col], (unsigned long long)deg);
                            } else {
                                atomicAdd(&a.sel_reads[col], 1u);
                                if (deg) atomicAdd(&a.sel_degree[col], (unsigned long long)deg);
                            }
                        }
                    }
                }
            }
            if (!any || cs > ce) continue;
            const uint32_t w0 = (cs - 1) >> 5, w1 = (ce - 1) >> 5;
            for (uint32_t wb = w0; wb <= w1; wb += 64) {
                const uint32_t wi = wb + lane;
                uint32_t mask = 0;
                if (wi <= w1) {
                    const uint32_t lo = wi == w0 ? (cs - 1) & 31u : 0u, hi = wi == w1 ? (ce - 1) & 31u : 31u;
                    mask = (0xFFFFFFFFu >> (31u - hi)) & (0xFFFFFFFFu << lo);
                }
                for (uint32_t j = 0; j < rv.n; j++) {           // no coverage where the read says N
                    const uint32_t w = a.read_word[rv.off0 + j];
                    if (((w >> 24) & 15u) != 15u) continue;
                    const uint32_t bit = (w & 0xFFFFFu) - 1u;
                    if ((bit >> 5) == wi) mask &= ~(1u << (bit & 31u));
                }
                if (!__ballot(mask != 0)) continue;
#pragma unroll
                for (uint32_t i = 0; i < ASG_REG_SLABS * 4; i++) {
                    unsigned long long b = ball[i];
                    while (b) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(b);
                        b &= b - 1;
                        const uint32_t col = (g * ASG_REG_SLABS + i / 4) * ASG_SLAB + l * ASG_LANE_HAPS + (i & 3u);
                        if (mask && col < a.K) {
                            uint32_t* p = a.cover + (size_t)col * a.cover_words + wi;
                            // (a stale word only costs an atomic that sets nothing new)
                            const uint32_t old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (mask & ~old) atomicOr(p, mask);
                        }
                    }
                }
            }
        }
        if (lane == 0) {
            a.min_dist[r] = best;
            a.n_epp[r] = ties;
        }
    }
    if (LDS_AGG) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < a.K; i += blockDim.x) {
            const uint32_t c = l_cnt[i];
            if (c) {
                atomicAdd(&a.sel_reads[i], c);
                if (l_deg[i]) atomicAdd(&a.sel_degree[i], l_deg[i]);
            }
        }
    }
}

// a wave per read: a lane's place in the list = ties of the slabs before + ties of the lanes below in its slab
__global__ void k_assign_lists(const unsigned long long* __restrict__ ties, const unsigned long long* __restrict__ asg_off,
                               uint32_t R, uint32_t nslabs, uint32_t* __restrict__ asg_sel) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < R; r += nwaves) {
        unsigned long long at = asg_off[r];
        const unsigned long long end = asg_off[r + 1];
        for (uint32_t slab = 0; slab < nslabs; slab++) {
            const unsigned long long* t = ties + ((size_t)r * nslabs + slab) * 4;
            const unsigned long long b0 = t[0], b1 = t[1], b2 = t[2], b3 = t[3];
            unsigned long long mine = at + __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below) + __popcll(b3 & below);
            const uint32_t col = slab * ASG_SLAB + lane * ASG_LANE_HAPS;
            if (((b0 >> lane) & 1ull) && mine < end) asg_sel[mine++] = col;
            if (((b1 >> lane) & 1ull) && mine < end) asg_sel[mine++] = col + 1;
            if (((b2 >> lane) & 1ull) && mine < end) asg_sel[mine++] = col + 2;
            if (((b3 >> lane) & 1ull) && mine < end) asg_sel[mine++] = col + 3;
            at += __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
        }
    }
}

__global__ void k_assign_popcount(const uint32_t* __restrict__ cover, uint32_t cover_words, uint32_t* __restrict__ sel_covered) {
    __shared__ uint32_t part[4];
    const uint32_t* row = cover + (size_t)blockIdx.x * cover_words;
    uint32_t s = 0;
    for (uint32_t i = threadIdx.x; i < cover_words; i += blockDim.x) s += (uint32_t)__popc(row[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sel_covered[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

struct WidenU32 {
    __host__ __device__ unsigned long long operator()(uint32_t v) const { return v; }
};

}  // namespace

hipError_t launch_assign_tables(const uint32_t* node_woff, const uint32_t* words, const uint32_t* parent_dfs,
                                const uint32_t* sel, uint32_t K, uint32_t Kp, uint32_t max_pos, uint8_t* geno,
                                uint16_t* pre, uint32_t* block_sums, uint32_t* overflow, hipStream_t stream) {
    const uint32_t rows = max_pos + 1, nblk = (rows + ASG_SCAN_ROWS - 1) / ASG_SCAN_ROWS;
    hipLaunchKernelGGL(k_assign_geno, dim3((K + 63) / 64), dim3(64), 0, stream, node_woff, words, parent_dfs, sel, K, Kp,
                       max_pos, geno);
    const dim3 grid((Kp / 4 + 255) / 256, nblk);
    hipLaunchKernelGGL(k_assign_count, grid, dim3(256), 0, stream, geno, Kp, rows, block_sums);
    hipLaunchKernelGGL(k_assign_blockscan, dim3((Kp + 255) / 256), dim3(256), 0, stream, block_sums, Kp, nblk, overflow);
    hipLaunchKernelGGL(k_assign_pre, grid, dim3(256), 0, stream, (const uint8_t*)geno, Kp, rows, (const uint32_t*)block_sums, pre);
    return hipGetLastError();
}

hipError_t launch_assign(const AssignArgs& a, hipStream_t stream) {
    if (a.R == 0) return hipSuccess;
    const uint32_t wgs = std::min<uint32_t>(ASG_MAX_WGS, (a.R + ASG_WAVES - 1) / ASG_WAVES);
    if (a.Kp <= ASG_LDS_MAX_COLS)
        hipLaunchKernelGGL(k_assign<true>, dim3(wgs), dim3(64 * ASG_WAVES), (size_t)a.Kp * 12, stream, a);
    else
        hipLaunchKernelGGL(k_assign<false>, dim3(wgs), dim3(64 * ASG_WAVES), 0, stream, a);
    return hipGetLastError();
}

hipError_t assign_scan_temp_bytes(uint32_t R, size_t* bytes) {
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, rocprim::make_transform_iterator((const uint32_t*)nullptr, WidenU32()),
                                   (unsigned long long*)nullptr, 0ull, (size_t)R + 1, rocprim::plus<unsigned long long>(), nullptr);
}

// n_epp holds R + 1 counts, the last one 0: the scan's last output is the total
hipError_t launch_assign_scan(const uint32_t* n_epp, unsigned long long* asg_off, uint32_t R, void* temp,
                              size_t temp_bytes, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, temp_bytes, rocprim::make_transform_iterator(n_epp, WidenU32()), asg_off, 0ull,
                                   (size_t)R + 1, rocprim::plus<unsigned long long>(), stream);
}

hipError_t launch_assign_lists(const unsigned long long* ties, const unsigned long long* asg_off, uint32_t R,
                               uint32_t Kp, uint32_t* asg_sel, hipStream_t stream) {
    if (R == 0) return hipSuccess;
    const uint32_t wgs = std::min<uint32_t>(ASG_MAX_WGS, (R + 3) / 4);
    hipLaunchKernelGGL(k_assign_lists, dim3(wgs), dim3(256), 0, stream, ties, asg_off, R, Kp / ASG_SLAB, asg_sel);
    return hipGetLastError();
}

hipError_t launch_assign_popcount(const uint32_t* cover, uint32_t K, uint32_t cover_words, uint32_t* sel_covered,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(k_assign_popcount, dim3(K), dim3(256), 0, stream, cover, cover_words, sel_covered);
    return hipGetLastError();
}

}  // namespace wepp
