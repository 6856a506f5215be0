// peaks_kernels.hip -- the device side of wepp_epp_peaks (the peak-removal loop of wepp_filter,
// src/WEPP/initial_filter.cpp:241-453) that is not already a kernel of the map or of the neighbour sets:
//   k_peak_max / k_peak_ties  the leader of a step: the largest full score over the live haplotypes and the
//                             haplotypes within eps of it (step(), :396-415)
//   k_peak_gather             the distances of the tie group to an accepted peak, out of its distance field
//   k_peak_mark               a region list -> mapped (clear_neighbors, :369-385)
//   k_peak_hits               the remaining reads an accepted peak corresponds to (find_correspondents, :241-282):
//                             d(read, peak) == max_parsimony with d in the closed form of assign_kernels.hip
//   k_peak_negq               the stored score shares of a subset of reads, negated (remove_read, :309-340)
// All of it is streaming integer work bound by memory; every launch is sized from a count the host holds, no
// kernel waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "peaks.hpp"

namespace wepp {

namespace {

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// the full score of haplotype i when it is live, -1 otherwise (a live one has score > eps > 0: never negative)
__device__ __forceinline__ double live_full(uint32_t i, const double* __restrict__ score, const double* __restrict__ divergence,
                                            const uint8_t* __restrict__ mapped, double eps) {
    if (mapped[i]) return -1.0;
    const double s = score[i];
    if (!(s > eps)) return -1.0;
    const double f = s * sqrt(divergence[i]);
    return f >= 0.0 ? f : -1.0;         // (a NaN divergence -- no bin holds a read -- is not a candidate)
}

}  // namespace

__global__ __launch_bounds__(PEAK_BLOCK) void k_peak_max(uint32_t N, const double* __restrict__ score,
                                                         const double* __restrict__ divergence,
                                                         const uint8_t* __restrict__ mapped, double eps, PeakTop* top) {
    double best = -1.0;
    uint32_t live = 0;
    for (uint32_t i = blockIdx.x * PEAK_BLOCK + threadIdx.x; i < N; i += gridDim.x * PEAK_BLOCK) {
        const double f = live_full(i, score, divergence, mapped, eps);
        live += f >= 0.0;
        best = fmax(best, f);
    }
    best = wave_max_f64(best);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) live += __shfl_xor(live, o);
    if ((threadIdx.x & 63u) == 0 && live) {
        // non-negative doubles order like their bit patterns
        atomicMax(&top->m_bits, (unsigned long long)__double_as_longlong(best));
        atomicAdd(&top->n_live, live);
    }
}

__global__ __launch_bounds__(PEAK_BLOCK) void k_peak_ties(uint32_t N, const double* __restrict__ score,
                                                          const double* __restrict__ divergence,
                                                          const uint8_t* __restrict__ mapped, double eps, PeakTop* top,
                                                          uint32_t* __restrict__ group, double* __restrict__ group_full) {
    const double m = __longlong_as_double((long long)top->m_bits);
    const uint32_t lane = threadIdx.x & 63u;
    // whole waves stay in the loop together: the ballot needs every lane
    const uint32_t n_round = (N + PEAK_BLOCK - 1) / PEAK_BLOCK * PEAK_BLOCK;
    for (uint32_t i = blockIdx.x * PEAK_BLOCK + threadIdx.x; i < n_round; i += gridDim.x * PEAK_BLOCK) {
        double f = -1.0;
        if (i < N) f = live_full(i, score, divergence, mapped, eps);
        const bool tie = f >= 0.0 && m - f < eps;
        const unsigned long long b = __ballot(tie);
        if (!b) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&top->n_tie, (uint32_t)__popcll(b));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (tie) {
            const uint32_t at = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            if (at < N) { group[at] = i; group_full[at] = f; }
        }
    }
}

__global__ __launch_bounds__(PEAK_BLOCK) void k_peak_gather(const int32_t* __restrict__ field, uint32_t Es, uint32_t col, uint32_t N,
                                                            const uint32_t* __restrict__ group, uint32_t n, int32_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * PEAK_BLOCK + threadIdx.x; i < n; i += gridDim.x * PEAK_BLOCK) {
        const uint32_t g = group[i];
        out[i] = g < N ? field[(size_t)g * Es + col] : INT32_MAX;
    }
}

__global__ __launch_bounds__(PEAK_BLOCK) void k_peak_mark(const uint32_t* __restrict__ nodes, uint64_t n, uint32_t N, uint8_t* mapped) {
    for (uint64_t i = (uint64_t)blockIdx.x * PEAK_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * PEAK_BLOCK) {
        const uint32_t nd = nodes[i];
        if (nd < N) mapped[nd] = 1;
    }
}

__global__ __launch_bounds__(PEAK_BLOCK) void k_peak_hits(PeakHitsArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r_round = (a.R + PEAK_BLOCK - 1) / PEAK_BLOCK * PEAK_BLOCK;
    for (uint32_t s = blockIdx.x * PEAK_BLOCK + threadIdx.x; s < r_round; s += gridDim.x * PEAK_BLOCK) {
        bool hit = false;
        if (s < a.R && a.alive[s]) {
            const uint32_t r = a.order[s];
            const uint32_t off0 = a.read_off[r], n = a.read_off[r + 1] - off0;
            const uint32_t st = (uint32_t)a.start[r], en = (uint32_t)a.end[r];
            const int32_t want = a.best[s];
            const size_t rowE = (size_t)min(en, a.max_pos) * a.Kp, rowS = (size_t)min(st - 1, a.max_pos) * a.Kp;
            int32_t not_n = 0;
            for (uint32_t j = 0; j < n; j++) not_n += ((a.read_word[off0 + j] >> 24) & 15u) != 15u;
            for (uint32_t k = 0; k < a.K && !hit; k++) {
                // every position of the window where the peak differs from the reference costs one, every listed
                // allele that is not N costs one, and where both meet the pair costs 0 (N or equal) or 1
                int32_t d = (int32_t)a.pre[rowE + k] - (int32_t)a.pre[rowS + k] + not_n;
                for (uint32_t j = 0; j < n; j++) {
                    const uint32_t w = a.read_word[off0 + j];
                    const uint32_t pos = w & 0xFFFFFu, mut = (w >> 24) & 15u;
                    if (pos < st || pos > en || pos > a.max_pos) continue;
                    const uint32_t g = a.geno[(size_t)pos * a.Kp + k];
                    if (g) d -= 1 + (int32_t)(mut != 15u && mut == g);
                }
                if (d == want) {
                    hit = true;
                    a.alive[s] = 0;
                    a.removed_step[r] = a.step;
                    a.removed_peak[r] = a.peak_base + k;
                    atomicAdd(&a.peak_reads[a.peak_base + k], 1u);
                    const int32_t deg = a.degree[r];
                    if (deg) atomicAdd(&a.peak_degree[a.peak_base + k], (unsigned long long)deg);
                }
            }
        }
        // the removed reads, compacted: one atomic per wave
        const unsigned long long b = __ballot(hit);
        if (!b) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(a.n_hits, (uint32_t)__popcll(b));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (hit) {
            const uint32_t at = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            if (at < a.R) a.hits[at] = s;
        }
    }
}

__global__ __launch_bounds__(PEAK_BLOCK) void k_peak_negq(uint32_t n, const uint32_t* __restrict__ places, const long long* __restrict__ q,
                                                          long long* __restrict__ out) {
    for (uint32_t i = blockIdx.x * PEAK_BLOCK + threadIdx.x; i < n; i += gridDim.x * PEAK_BLOCK) out[i] = -q[places[i]];
}

// ---- launchers ---------------------------------------------------------------------------------------------
static uint32_t peak_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + PEAK_BLOCK - 1) / PEAK_BLOCK, 1), PEAK_MAX_WGS); }

hipError_t launch_peak_max(uint32_t N, const double* score, const double* divergence, const uint8_t* mapped, double eps,
                           PeakTop* top, hipStream_t stream) {
    hipLaunchKernelGGL(k_peak_max, dim3(peak_grid(N)), dim3(PEAK_BLOCK), 0, stream, N, score, divergence, mapped, eps, top);
    return hipGetLastError();
}
hipError_t launch_peak_ties(uint32_t N, const double* score, const double* divergence, const uint8_t* mapped, double eps,
                            PeakTop* top, uint32_t* group, double* group_full, hipStream_t stream) {
    hipLaunchKernelGGL(k_peak_ties, dim3(peak_grid(N)), dim3(PEAK_BLOCK), 0, stream, N, score, divergence, mapped, eps, top, group, group_full);
    return hipGetLastError();
}
hipError_t launch_peak_gather(const int32_t* field, uint32_t Es, uint32_t col, uint32_t N, const uint32_t* group, uint32_t n,
                              int32_t* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_peak_gather, dim3(peak_grid(n)), dim3(PEAK_BLOCK), 0, stream, field, Es, col, N, group, n, out);
    return hipGetLastError();
}
hipError_t launch_peak_mark(const uint32_t* nodes, uint64_t n, uint32_t N, uint8_t* mapped, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_peak_mark, dim3(peak_grid(n)), dim3(PEAK_BLOCK), 0, stream, nodes, n, N, mapped);
    return hipGetLastError();
}
hipError_t launch_peak_hits(const PeakHitsArgs& a, hipStream_t stream) {
    if (a.R == 0 || a.K == 0) return hipSuccess;
    hipLaunchKernelGGL(k_peak_hits, dim3(peak_grid(a.R)), dim3(PEAK_BLOCK), 0, stream, a);
    return hipGetLastError();
}
hipError_t launch_peak_negq(uint32_t n, const uint32_t* places, const long long* q, long long* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_peak_negq, dim3(peak_grid(n)), dim3(PEAK_BLOCK), 0, stream, n, places, q, out);
    return hipGetLastError();
}

}  // namespace wepp
