// clades_kernels.hip -- clade assignment of placed samples: the loop the reference marks "can be parallelized"
// (usher_common.cpp:603-615) over every (read, optimal node) pair of a batch, then the sorted clade lists of
// Missing_Sample::clade_assignments as run-length histograms (what the -D writer prints, :937-954).
//
//   k_clade_pairs       lane = pair.  The read of a pair comes from a binary search in the CSR of the pairs, so one
//                       read with 100 000 pairs and 100 000 reads with one pair each fill the same grid; neighbouring
//                       lanes share a read (its entries are broadcast loads) and differ in the node.  has_unique is
//                       node_has_unique (place_dev.hpp): a loop over the node's own mutation words with a binary search
//                       in the read's entries -- lanes diverge by the nodes' mutation counts (a handful on real trees);
//                       then two table lookups per column.  Bound by the scattered loads of nstat / node_woff / words.
//   k_clade_sort_wave   segments of 2 .. 64 keys: one wave, one key per lane, a bitonic network on lane exchanges.
//   k_clade_sort_block  segments of 65 .. 1024 keys: one workgroup, a bitonic network in 4 KiB of LDS.
//   long segments       gathered as (segment << 32 | clade), one device radix sort (rocPRIM), scattered back.
//   k_clade_heads ..    run heads of the sorted keys, their exclusive scan (rocPRIM), offsets, run starts, counts: the
//                       same kernels whatever sorted a segment, so the result cannot depend on the path.
// Integer work only; every index is bounded by values the host has checked (clades_capi.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "clades.hpp"
#include "place_dev.hpp"

namespace wepp {

namespace {

// largest i in [0, n) with off[i] <= x; off[0] <= x < off[n]
__device__ __forceinline__ uint32_t csr_find(const uint32_t* __restrict__ off, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_clade_pairs(DevMAT m, CladeArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.P) return;
    const uint32_t r = csr_find(a.best_off, a.R, p);
    const uint32_t bfs_j = a.best_nodes[p];
    const uint32_t d = m.bfs2dfs[bfs_j];
    const uint32_t so = a.read_off[r];
    const uint32_t hu = node_has_unique(m, d, a.read_word, so, a.read_off[r + 1] - so);
    const uint32_t include_self = (!(m.nstat[d] & NS_LEAF_DEV) && !hu) ? 1u : 0u;          // usher_common.cpp:607
    const bool single = a.best_off[r + 1] - a.best_off[r] == 1u;
    const bool is_best = bfs_j == a.best_bfs_j[r];                                          // :610
    a.pair_read[p] = r;
    for (uint32_t c = 0; c < a.C; c++) {
        const uint32_t v = a.tab[((size_t)c * 2 + include_self) * m.N + d];
        a.keys[c * a.P + p] = v;
        if (single) a.sorted[c * a.P + p] = v;
        if (is_best) a.best_clade[(size_t)c * a.R + r] = v;
    }
    if (is_best) a.found[r] = 1u;
}

__global__ __launch_bounds__(256) void k_clade_sort_wave(CladeArgs a, const uint32_t* __restrict__ list, uint32_t n) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= n * a.C) return;
    const uint32_t c = w / n, r = list[w % n];
    const uint32_t off = a.best_off[r], L = a.best_off[r + 1] - off;
    const uint32_t at = c * a.P + off + lane;
    uint32_t v = lane < L ? a.keys[at] : 0xFFFFFFFFu;
    for (uint32_t k = 2; k <= 64; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t o = __shfl_xor(v, (int)j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            v = keep_min ? min(v, o) : max(v, o);
        }
    if (lane < L) a.sorted[at] = v;
}

__global__ __launch_bounds__(CLADE_BLOCK_THREADS) void k_clade_sort_block(CladeArgs a, const uint32_t* __restrict__ list, uint32_t n) {
    __shared__ uint32_t s[CLADE_BLOCK_MAX];
    const uint32_t c = blockIdx.x / n, r = list[blockIdx.x % n], tid = threadIdx.x;
    const uint32_t off = a.best_off[r], L = min(a.best_off[r + 1] - off, CLADE_BLOCK_MAX);
    const uint32_t base = c * a.P + off;
    uint32_t n2 = 128;
    while (n2 < L) n2 <<= 1;
    for (uint32_t t = tid; t < n2; t += CLADE_BLOCK_THREADS) s[t] = t < L ? a.keys[base + t] : 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t k = 2; k <= n2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < n2 / 2; t += CLADE_BLOCK_THREADS) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));     // the lower element of the t-th pair at distance j
                const uint32_t x = s[i], y = s[i + j];
                if ((x > y) == ((i & k) == 0)) { s[i] = y; s[i + j] = x; }
            }
            __syncthreads();
        }
    for (uint32_t t = tid; t < L; t += CLADE_BLOCK_THREADS) a.sorted[base + t] = s[t];
}

// element e of the long segments' key array: column e / n_long_pairs, read list[i] with long_off[i] <= e % n_long_pairs
__device__ __forceinline__ uint32_t long_source(const CladeArgs& a, const uint32_t* __restrict__ list, const uint32_t* __restrict__ long_off,
                                                uint32_t n, uint32_t n_long_pairs, uint32_t e, uint32_t& seg) {
    const uint32_t c = e / n_long_pairs, jj = e % n_long_pairs;
    const uint32_t i = csr_find(long_off, n, jj);
    seg = c * n + i;
    return c * a.P + a.best_off[list[i]] + (jj - long_off[i]);
}
__global__ __launch_bounds__(256) void k_clade_long_gather(CladeArgs a, const uint32_t* __restrict__ list, const uint32_t* __restrict__ long_off,
                                                           uint32_t n, uint32_t n_long_pairs, unsigned long long* __restrict__ key64) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= a.C * n_long_pairs) return;
    uint32_t seg;
    const uint32_t src = long_source(a, list, long_off, n, n_long_pairs, e, seg);
    key64[e] = ((unsigned long long)seg << 32) | a.keys[src];
}
__global__ __launch_bounds__(256) void k_clade_long_scatter(CladeArgs a, const uint32_t* __restrict__ list, const uint32_t* __restrict__ long_off,
                                                            uint32_t n, uint32_t n_long_pairs, const unsigned long long* __restrict__ key64) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= a.C * n_long_pairs) return;
    uint32_t seg;
    const uint32_t dst = long_source(a, list, long_off, n, n_long_pairs, e, seg);
    a.sorted[dst] = (uint32_t)key64[e];       // (the sort keeps the segments' sizes and order: place e is still segment seg's)
}

__global__ __launch_bounds__(256) void k_clade_heads(CladeArgs a, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.C * a.P) return;
    const uint32_t p = i % a.P;
    const bool first = p == a.best_off[a.pair_read[p]];
    head[i] = (first || a.sorted[i] != a.sorted[i - 1]) ? 1u : 0u;
}
// hist_off[s] for segment s = column * R + read: the runs before the segment's first key; hist_off[C * R] = all runs
__global__ __launch_bounds__(256) void k_clade_offsets(CladeArgs a, const uint32_t* __restrict__ run_of, unsigned long long* __restrict__ hist_off) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > a.C * a.R) return;
    const uint32_t e = s == a.C * a.R ? a.C * a.P : (s / a.R) * a.P + a.best_off[s % a.R];
    hist_off[s] = run_of[e];
}
__global__ __launch_bounds__(256) void k_clade_run_starts(CladeArgs a, const uint32_t* __restrict__ head, const uint32_t* __restrict__ run_of,
                                                          uint32_t n_runs, uint32_t* __restrict__ run_start, uint32_t* __restrict__ hist_clade) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > a.C * a.P) return;
    if (i == a.C * a.P) { run_start[n_runs] = i; return; }
    if (!head[i]) return;
    const uint32_t run = run_of[i];
    run_start[run] = i;
    if (hist_clade) hist_clade[run] = a.sorted[i];
}
__global__ __launch_bounds__(256) void k_clade_run_counts(const uint32_t* __restrict__ run_start, uint32_t n_runs, uint32_t* __restrict__ hist_count) {
    const uint32_t run = blockIdx.x * 256u + threadIdx.x;
    if (run < n_runs) hist_count[run] = run_start[run + 1] - run_start[run];
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + 255) / 256); }

}  // namespace

hipError_t launch_clade_pairs(const DevMAT& m, const CladeArgs& a, hipStream_t stream) {
    if (a.P == 0) return hipSuccess;
    hipLaunchKernelGGL(k_clade_pairs, dim3(blocks_of(a.P)), dim3(256), 0, stream, m, a);
    return hipGetLastError();
}

hipError_t launch_clade_sort_wave(const CladeArgs& a, const uint32_t* list, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_clade_sort_wave, dim3((uint32_t)(((uint64_t)n * a.C + 3) / 4)), dim3(256), 0, stream, a, list, n);
    return hipGetLastError();
}

hipError_t launch_clade_sort_block(const CladeArgs& a, const uint32_t* list, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_clade_sort_block, dim3(n * a.C), dim3(CLADE_BLOCK_THREADS), 0, stream, a, list, n);
    return hipGetLastError();
}

hipError_t clade_sort_long_temp_bytes(uint64_t n_keys, uint32_t end_bit, size_t* bytes) {
    *bytes = 0;
    return rocprim::radix_sort_keys(nullptr, *bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, n_keys, 0,
                                    end_bit, nullptr);
}

hipError_t launch_clade_sort_long(const CladeArgs& a, const uint32_t* list, const uint32_t* long_off, uint32_t n,
                                  uint32_t n_long_pairs, unsigned long long* key64, unsigned long long* key64_out,
                                  uint32_t end_bit, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n == 0 || n_long_pairs == 0) return hipSuccess;
    const uint64_t n_keys = (uint64_t)a.C * n_long_pairs;
    hipLaunchKernelGGL(k_clade_long_gather, dim3(blocks_of(n_keys)), dim3(256), 0, stream, a, list, long_off, n, n_long_pairs, key64);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_keys(temp, temp_bytes, (const unsigned long long*)key64, key64_out, n_keys, 0, end_bit, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_clade_long_scatter, dim3(blocks_of(n_keys)), dim3(256), 0, stream, a, list, long_off, n, n_long_pairs,
                       (const unsigned long long*)key64_out);
    return hipGetLastError();
}

hipError_t clade_scan_temp_bytes(uint64_t n, size_t* bytes) {
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), nullptr);
}

// head holds C * P + 1 words, the last one zeroed here: the scan's last output is the number of runs
hipError_t launch_clade_heads(const CladeArgs& a, uint32_t* head, uint32_t* run_of, unsigned long long* hist_off, void* temp,
                              size_t temp_bytes, hipStream_t stream) {
    const uint64_t n = (uint64_t)a.C * a.P;
    hipError_t e = hipMemsetAsync(head + n, 0, 4, stream);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(k_clade_heads, dim3(blocks_of(n)), dim3(256), 0, stream, a, head);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)head, run_of, 0u, n + 1, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_clade_offsets, dim3(blocks_of((uint64_t)a.C * a.R + 1)), dim3(256), 0, stream, a, (const uint32_t*)run_of, hist_off);
    return hipGetLastError();
}

hipError_t launch_clade_runs(const CladeArgs& a, const uint32_t* head, const uint32_t* run_of, uint32_t n_runs,
                             uint32_t* run_start, uint32_t* hist_clade, uint32_t* hist_count, hipStream_t stream) {
    hipLaunchKernelGGL(k_clade_run_starts, dim3(blocks_of((uint64_t)a.C * a.P + 1)), dim3(256), 0, stream, a, head, run_of, n_runs, run_start,
                       hist_clade);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !hist_count || n_runs == 0) return e;
    hipLaunchKernelGGL(k_clade_run_counts, dim3(blocks_of(n_runs)), dim3(256), 0, stream, (const uint32_t*)run_start, n_runs, hist_count);
    return hipGetLastError();
}

}  // namespace wepp
