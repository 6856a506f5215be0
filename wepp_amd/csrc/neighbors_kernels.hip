// neighbors_kernels.hip -- wepp_epp_neighbors: the haplotypes within a mutation radius of PIVOTS, reachable through
// haplotypes that are within it too (arena::closest_neighbors and arena::highest_scoring_neighbors,
// src/WEPP/arena.cpp:171-249, over haplotype::mutation_distance(haplotype*), src/WEPP/haplotype.hpp:179).
//
// The distance of a pivot to every node is a path sum, not one list merge per node.  With g the pivot's allele at a
// position (0 = reference) and t the node's, a position costs
//   form TO   (node->mutation_distance(pivot)):  [g != 15] * [t != g]
//   form FROM (pivot->mutation_distance(node)):  [t != 15] * [t != g]
// A mutation word of a node changes t from `old` to `new` at one position for the node's whole subtree, so it adds
// cost(new) - cost(old) to every distance of the pre-order rows [n, dfs_end(n)): +delta at row n, -delta at row
// dfs_end(n) of a table of N + 1 rows, whose inclusive scan down the columns is the distance field; row 0 also
// starts from the distance of the reference genome.  The pivots' genotypes are the position-major table of
// wepp_epp_assign (assign_kernels.hip): a wave takes a node, a lane 4 pivot columns -- one dword of a table row per
// word -- compared byte-wise.  The count of nodes beyond the radius on the root path is a second path sum through
// the same scan; a node is in the component of the pivot iff it lies in the subtree of the component's top and has
// the top's count.  Everything is integer; the atomics are integer additions, so no result depends on their order,
// and the lists are placed by counts, not by arrival.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "neighbors.hpp"

namespace wepp {

namespace {

constexpr uint32_t NBR_NIB = 0x0F0F0F0Fu, NBR_ONES = 0x01010101u;
// bytes hold values 0 .. 15: 1 in every byte that is not zero
__device__ __forceinline__ uint32_t nbr_nz(uint32_t v) { return ((v + NBR_NIB) >> 4) & NBR_ONES; }

struct alignas(16) Cell4 { uint32_t v[4]; };    // the 4 columns of a thread in one row

// the row tables are walked by threads that own 4 columns and NBR_SCAN_ROWS rows: blockIdx.x = block of rows,
// blockIdx.y * blockDim.x + threadIdx.x = group of 4 columns
__device__ __forceinline__ uint32_t my_col() { return (blockIdx.y * blockDim.x + threadIdx.x) * NBR_LANE_COLS; }

// ---- the distance of the reference genome: the pivot's positions that cost against allele 0 ---------------------
__global__ void k_nbr_base(const uint8_t* __restrict__ geno, uint32_t Kp, uint32_t Es, uint32_t rows, int form, int32_t* field) {
    const uint32_t c = my_col();
    if (c >= Es) return;
    const uint32_t r0 = blockIdx.x * NBR_SCAN_ROWS, r1 = min(rows, r0 + NBR_SCAN_ROWS);
    uint32_t s[4] = {0, 0, 0, 0};
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t g4 = *(const uint32_t*)(geno + (size_t)r * Kp + c);
        uint32_t cost = nbr_nz(g4);                                            // t = 0: [0 != g]
        if (form == 0) cost &= nbr_nz(g4 ^ NBR_NIB);                           // ... and [g != 15]
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) s[j] += (cost >> (8 * j)) & 1u;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
        if (s[j]) atomicAdd(&field[c + j], (int32_t)s[j]);
}

// ---- the deltas of the mutation words -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nbr_delta(NbrTree t, const uint8_t* __restrict__ geno, uint32_t Kp, uint32_t Es, int form,
                                                   int32_t* field) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t n = blockIdx.x * (blockDim.x >> 6) + wave; n < t.N; n += nwaves) {
        const uint32_t w0 = __builtin_amdgcn_readfirstlane(t.node_woff[n]), w1 = __builtin_amdgcn_readfirstlane(t.node_woff[n + 1]);
        if (w0 == w1) continue;
        const uint32_t end = __builtin_amdgcn_readfirstlane(t.dfs_end[n]);
        for (uint32_t c = lane * NBR_LANE_COLS; c < Es; c += NBR_SLAB) {
            int32_t d[4] = {0, 0, 0, 0};
            for (uint32_t w = w0; w < w1; w++) {
                const uint32_t word = t.words[w];
                const uint32_t pos = word & 0xFFFFFu;
                if (pos > t.max_pos) continue;
                const uint32_t ref = 1u << ((word >> 20) & 3u), par = (word >> 22) & 15u, mut = (word >> 26) & 15u;
                const uint32_t was = (par == 0 || par == ref) ? 0u : par, now = mut == ref ? 0u : mut;
                if (was == now) continue;
                const uint32_t g4 = *(const uint32_t*)(geno + (size_t)pos * Kp + c);
                uint32_t a = nbr_nz(g4 ^ (now * NBR_ONES)), b = nbr_nz(g4 ^ (was * NBR_ONES));
                if (form == 0) {
                    const uint32_t known = nbr_nz(g4 ^ NBR_NIB);
                    a &= known; b &= known;
                } else {
                    if (now == 15u) a = 0;
                    if (was == 15u) b = 0;
                }
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) d[j] += (int32_t)((a >> (8 * j)) & 1u) - (int32_t)((b >> (8 * j)) & 1u);
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                if (d[j]) {
                    atomicAdd(&field[(size_t)n * Es + c + j], d[j]);
                    atomicAdd(&field[(size_t)end * Es + c + j], -d[j]);
                }
        }
    }
}

// ---- inclusive scan down the columns, blocked as k_assign_count / _blockscan / _pre ---------------------------
__global__ void k_nbr_colsum(const uint32_t* __restrict__ table, uint32_t Es, uint32_t rows, uint32_t* __restrict__ block_sums) {
    const uint32_t c = my_col();
    if (c >= Es) return;
    const uint32_t r0 = blockIdx.x * NBR_SCAN_ROWS, r1 = min(rows, r0 + NBR_SCAN_ROWS);
    Cell4 s = {{0, 0, 0, 0}};
    for (uint32_t r = r0; r < r1; r++) {
        const Cell4 v = *(const Cell4*)(table + (size_t)r * Es + c);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) s.v[j] += v.v[j];
    }
    *(Cell4*)(block_sums + (size_t)blockIdx.x * Es + c) = s;
}

// block_sums <- its exclusive scan down the blocks; totals (or nullptr) <- the column sums
__global__ void k_nbr_blockscan(uint32_t* block_sums, uint32_t Es, uint32_t nblk, uint32_t* totals) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Es) return;
    uint32_t run = 0;
    for (uint32_t b = 0; b < nblk; b++) {
        const uint32_t v = block_sums[(size_t)b * Es + c];
        block_sums[(size_t)b * Es + c] = run;
        run += v;
    }
    if (totals) totals[c] = run;
}

__global__ void k_nbr_colscan(uint32_t* table, uint32_t Es, uint32_t rows, const uint32_t* __restrict__ block_sums) {
    const uint32_t c = my_col();
    if (c >= Es) return;
    const uint32_t r0 = blockIdx.x * NBR_SCAN_ROWS, r1 = min(rows, r0 + NBR_SCAN_ROWS);
    Cell4 s = *(const Cell4*)(block_sums + (size_t)blockIdx.x * Es + c);
    for (uint32_t r = r0; r < r1; r++) {
        Cell4* cell = (Cell4*)(table + (size_t)r * Es + c);
        const Cell4 v = *cell;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) s.v[j] += v.v[j];
        *cell = s;
    }
}

// ---- nodes beyond the radius, as deltas of the second path sum -----------------------------------------------
__global__ void k_nbr_over(uint32_t N, const uint32_t* __restrict__ dfs_end, const uint32_t* __restrict__ field, uint32_t Es,
                           uint32_t radius, int32_t* over) {
    const uint32_t c = my_col();
    if (c >= Es) return;
    const uint32_t r0 = blockIdx.x * NBR_SCAN_ROWS, r1 = min(N, r0 + NBR_SCAN_ROWS);
    for (uint32_t r = r0; r < r1; r++) {
        const Cell4 v = *(const Cell4*)(field + (size_t)r * Es + c);
        if (v.v[0] <= radius && v.v[1] <= radius && v.v[2] <= radius && v.v[3] <= radius) continue;
        const uint32_t end = dfs_end[r];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            if (v.v[j] > radius) {
                atomicAdd(&over[(size_t)r * Es + c + j], 1);
                atomicAdd(&over[(size_t)end * Es + c + j], -1);
            }
    }
}

// ---- the top of a pivot's component: climb while the parent is within the radius ---------------------------------
__global__ void k_nbr_tops(NbrTree t, const uint32_t* __restrict__ piv, uint32_t Kc, const uint32_t* __restrict__ field,
                           const int32_t* __restrict__ over, uint32_t Es, uint32_t radius, uint32_t* top, uint32_t* top_end,
                           int32_t* top_over) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Es) return;
    if (k >= Kc) {                      // padding columns: an empty range
        top[k] = 0xFFFFFFFFu; top_end[k] = 0; top_over[k] = 0;
        return;
    }
    uint32_t a = piv[k];
    while (a != 0) {
        const uint32_t p = t.parent_dfs[a];
        if (p >= a) break;              // (pre-order: a parent precedes its children)
        if (field[(size_t)p * Es + k] > radius) break;
        a = p;
    }
    top[k] = a; top_end[k] = t.dfs_end[a]; top_over[k] = over[(size_t)a * Es + k];
}

struct Range4 { uint32_t lo[4], hi[4]; int32_t want[4]; };

__device__ __forceinline__ bool load_ranges(uint32_t c, uint32_t r0, uint32_t r1, const uint32_t* top, const uint32_t* top_end,
                                            const int32_t* top_over, Range4& g) {
    bool any = false;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        g.lo[j] = top[c + j]; g.hi[j] = top_end[c + j]; g.want[j] = top_over[c + j];
        any |= g.lo[j] < r1 && g.hi[j] > r0;
    }
    return any;
}

// ---- members of the components per block of rows ----------------------------------------------------------------
__global__ void k_nbr_count(uint32_t N, const int32_t* __restrict__ over, uint32_t Es, const uint32_t* __restrict__ top,
                            const uint32_t* __restrict__ top_end, const int32_t* __restrict__ top_over,
                            const uint8_t* __restrict__ skip, uint32_t* __restrict__ block_counts, uint32_t* n_region) {
    const uint32_t c = my_col();
    if (c >= Es) return;
    const uint32_t r0 = blockIdx.x * NBR_SCAN_ROWS, r1 = min(N, r0 + NBR_SCAN_ROWS);
    Range4 g;
    Cell4 listed = {{0, 0, 0, 0}};
    uint32_t region[4] = {0, 0, 0, 0};
    if (load_ranges(c, r0, r1, top, top_end, top_over, g)) {
        for (uint32_t r = r0; r < r1; r++) {
            const Cell4 v = *(const Cell4*)(over + (size_t)r * Es + c);
            const uint32_t keep = skip ? (skip[r] == 0) : 1u;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t in = r >= g.lo[j] && r < g.hi[j] && (int32_t)v.v[j] == g.want[j];
                region[j] += in;
                listed.v[j] += in & keep;
            }
        }
    }
    *(Cell4*)(block_counts + (size_t)blockIdx.x * Es + c) = listed;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
        if (region[j]) atomicAdd(&n_region[c + j], region[j]);
}

// ---- the lists: a thread writes the members of its columns in row order from the block's place ----------------
__global__ void k_nbr_write(uint32_t N, uint32_t Kc, const int32_t* __restrict__ field, const int32_t* __restrict__ over, uint32_t Es,
                            const uint32_t* __restrict__ top, const uint32_t* __restrict__ top_end,
                            const int32_t* __restrict__ top_over, const uint8_t* __restrict__ skip,
                            const uint32_t* __restrict__ block_counts, const unsigned long long* __restrict__ off,
                            uint32_t* __restrict__ nbr_node, int32_t* __restrict__ nbr_dist) {
    const uint32_t c = my_col();
    if (c >= Kc) return;
    const uint32_t r0 = blockIdx.x * NBR_SCAN_ROWS, r1 = min(N, r0 + NBR_SCAN_ROWS);
    Range4 g;
    if (!load_ranges(c, r0, r1, top, top_end, top_over, g)) return;
    unsigned long long at[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) at[j] = (c + j < Kc ? off[c + j] : 0ull) + block_counts[(size_t)blockIdx.x * Es + c + j];
    for (uint32_t r = r0; r < r1; r++) {
        if (skip && skip[r]) continue;
        const Cell4 v = *(const Cell4*)(over + (size_t)r * Es + c);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            if (r >= g.lo[j] && r < g.hi[j] && (int32_t)v.v[j] == g.want[j]) {
                nbr_node[at[j]] = r;
                nbr_dist[at[j]] = field[(size_t)r * Es + c + j];
                at[j]++;
            }
    }
}

inline dim3 table_grid(uint32_t rows, uint32_t Es) { return dim3(nbr_scan_blocks(rows), (Es / NBR_LANE_COLS + 63) / 64); }

}  // namespace

hipError_t launch_nbr_deltas(const NbrTree& t, const uint8_t* geno, uint32_t Kp, uint32_t Es, int form, int32_t* field,
                             hipStream_t stream) {
    hipLaunchKernelGGL(k_nbr_base, table_grid(t.max_pos + 1, Es), dim3(64), 0, stream, geno, Kp, Es, t.max_pos + 1, form, field);
    const uint32_t wgs = std::min<uint32_t>(NBR_MAX_WGS, (t.N + 3) / 4);
    hipLaunchKernelGGL(k_nbr_delta, dim3(wgs), dim3(256), 0, stream, t, geno, Kp, Es, form, field);
    return hipGetLastError();
}

hipError_t launch_nbr_colscan(int32_t* table, uint32_t Es, uint32_t rows, uint32_t* block_sums, hipStream_t stream) {
    const dim3 grid = table_grid(rows, Es);
    hipLaunchKernelGGL(k_nbr_colsum, grid, dim3(64), 0, stream, (const uint32_t*)table, Es, rows, block_sums);
    hipLaunchKernelGGL(k_nbr_blockscan, dim3((Es + 255) / 256), dim3(256), 0, stream, block_sums, Es, grid.x, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_nbr_colscan, grid, dim3(64), 0, stream, (uint32_t*)table, Es, rows, (const uint32_t*)block_sums);
    return hipGetLastError();
}

hipError_t launch_nbr_over(const NbrTree& t, const int32_t* field, uint32_t Es, uint32_t radius, int32_t* over, hipStream_t stream) {
    hipLaunchKernelGGL(k_nbr_over, table_grid(t.N, Es), dim3(64), 0, stream, t.N, t.dfs_end, (const uint32_t*)field, Es, radius, over);
    return hipGetLastError();
}

hipError_t launch_nbr_tops(const NbrTree& t, const uint32_t* piv, uint32_t Kc, const int32_t* field, const int32_t* over,
                           uint32_t Es, uint32_t radius, uint32_t* top, uint32_t* top_end, int32_t* top_over, hipStream_t stream) {
    hipLaunchKernelGGL(k_nbr_tops, dim3((Es + 63) / 64), dim3(64), 0, stream, t, piv, Kc, (const uint32_t*)field, over, Es, radius,
                       top, top_end, top_over);
    return hipGetLastError();
}

hipError_t launch_nbr_count(uint32_t N, const int32_t* over, uint32_t Es, const uint32_t* top, const uint32_t* top_end,
                            const int32_t* top_over, const uint8_t* skip, uint32_t* block_counts, uint32_t* n_region,
                            uint32_t* n_listed, hipStream_t stream) {
    const dim3 grid = table_grid(N, Es);
    hipLaunchKernelGGL(k_nbr_count, grid, dim3(64), 0, stream, N, over, Es, top, top_end, top_over, skip, block_counts, n_region);
    hipLaunchKernelGGL(k_nbr_blockscan, dim3((Es + 255) / 256), dim3(256), 0, stream, block_counts, Es, grid.x, n_listed);
    return hipGetLastError();
}

hipError_t launch_nbr_write(uint32_t N, uint32_t Kc, const int32_t* field, const int32_t* over, uint32_t Es, const uint32_t* top,
                            const uint32_t* top_end, const int32_t* top_over, const uint8_t* skip, const uint32_t* block_counts,
                            const unsigned long long* off, uint32_t* nbr_node, int32_t* nbr_dist, hipStream_t stream) {
    hipLaunchKernelGGL(k_nbr_write, table_grid(N, Es), dim3(64), 0, stream, N, Kc, field, over, Es, top, top_end, top_over, skip,
                       block_counts, off, nbr_node, nbr_dist);
    return hipGetLastError();
}

}  // namespace wepp
