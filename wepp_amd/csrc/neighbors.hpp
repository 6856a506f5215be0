// neighbors.hpp -- haplotypes within a mutation radius of pivots (arena::closest_neighbors and
// arena::highest_scoring_neighbors, src/WEPP/arena.cpp:171-249): shared declarations of neighbors_kernels.hip
// and neighbors_capi.cpp.  See DESIGN.md section 4.8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wepp {

// A pass holds two tables of [N + 1] rows x `Es` columns of 32-bit cells: the distance field (deltas, then their
// column scan) and the count of nodes beyond the radius on the root path.  NBR_PASS_BYTES bounds the two together;
// the pivots of a call are cut into passes of as many columns as fit (a multiple of NBR_LANE_COLS, at least that).
constexpr uint64_t NBR_PASS_BYTES = 2ull << 30;
constexpr uint32_t NBR_LANE_COLS = 4;                 // columns a lane (and a thread of the scans) owns: one dword of a geno row
constexpr uint32_t NBR_SLAB = 64 * NBR_LANE_COLS;     // columns a wave covers per row load
constexpr uint32_t NBR_SCAN_ROWS = 256;               // rows per block of the column scans
constexpr uint32_t NBR_MAX_WGS = 8192;                // k_nbr_delta: the waves stride over the nodes
constexpr uint64_t NBR_MAX_FIELD_CELLS = 1ull << 28;  // wepp_epp_distances: n_piv * n_nodes (1 GiB of int32)

inline uint32_t nbr_stride(uint32_t cols) { return (cols + NBR_LANE_COLS - 1) / NBR_LANE_COLS * NBR_LANE_COLS; }
inline uint32_t nbr_scan_blocks(uint32_t rows) { return (rows + NBR_SCAN_ROWS - 1) / NBR_SCAN_ROWS; }

struct NbrTree {                  // device arrays of the handle
    uint32_t N, max_pos;
    const uint32_t* node_woff;
    const uint32_t* words;
    const uint32_t* parent_dfs;
    const uint32_t* dfs_end;      // [N] one past the last pre-order index of the subtree
};

// field[N + 1][Es] (zeroed by the caller) <- the delta of every mutation word against the pivots' genotypes
// geno[max_pos + 1][Kp], added at the node's row and taken off at row dfs_end; row 0 also receives the distance of
// the reference genome.  form: WEPP_NBR_TO_PIVOT (0) or WEPP_NBR_FROM_PIVOT (1).
hipError_t launch_nbr_deltas(const NbrTree& t, const uint8_t* geno, uint32_t Kp, uint32_t Es, int form, int32_t* field,
                             hipStream_t stream);
// table[rows][Es] <- its inclusive scan down the columns; block_sums: [nbr_scan_blocks(rows)][Es]
hipError_t launch_nbr_colscan(int32_t* table, uint32_t Es, uint32_t rows, uint32_t* block_sums, hipStream_t stream);
// over[N + 1][Es] (zeroed by the caller) <- +1 at row n, -1 at row dfs_end[n] for every cell of field beyond the radius
hipError_t launch_nbr_over(const NbrTree& t, const int32_t* field, uint32_t Es, uint32_t radius, int32_t* over,
                           hipStream_t stream);
// per pivot column k < Kc: top[k] <- the highest ancestor reached from piv[k] through nodes within the radius,
// top_end[k] <- dfs_end of it, top_over[k] <- over[top[k]][k]; columns Kc .. Es get an empty range
hipError_t launch_nbr_tops(const NbrTree& t, const uint32_t* piv, uint32_t Kc, const int32_t* field, const int32_t* over,
                           uint32_t Es, uint32_t radius, uint32_t* top, uint32_t* top_end, int32_t* top_over, hipStream_t stream);
// n_region[k] (zeroed by the caller) <- nodes of the component; block_counts[nbr_scan_blocks(N)][Es] <- those not
// skipped, per block of rows, then exclusively scanned down the blocks; n_listed[k] <- their total
hipError_t launch_nbr_count(uint32_t N, const int32_t* over, uint32_t Es, const uint32_t* top, const uint32_t* top_end,
                            const int32_t* top_over, const uint8_t* skip, uint32_t* block_counts, uint32_t* n_region,
                            uint32_t* n_listed, hipStream_t stream);
// nbr_node / nbr_dist [off[k] ..) <- the listed nodes of column k ascending, with their distances
hipError_t launch_nbr_write(uint32_t N, uint32_t Kc, const int32_t* field, const int32_t* over, uint32_t Es, const uint32_t* top,
                            const uint32_t* top_end, const int32_t* top_over, const uint8_t* skip, const uint32_t* block_counts,
                            const unsigned long long* off, uint32_t* nbr_node, int32_t* nbr_dist, hipStream_t stream);

}  // namespace wepp
