// clades_host.hpp -- the host half of wepp_mat_set_clades as plain functions (no HIP): the two ancestor tables of
// every annotation column.  Tree::get_clade_assignment (mutation_annotated_tree.cpp:923-931) walks rsearch(node,
// include_self) to the first annotated node; here both answers of every node are precomputed by one top-down pass.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace wepp {

// tab[(c * 2 + include_self) * N + d] for the node with DFS (pre-order) index d: the clade id of its nearest annotated
// ancestor excluding (0) / including (1) the node itself, undefined_id[c] when there is none.  parent_dfs[d] < d for
// d > 0 (pre-order), so one ascending pass sees every parent before its children.  clade_id is indexed by caller node
// id (dfs2id[d]), 0 = not annotated.
inline void clade_build_tables(uint32_t N, uint32_t C, const uint32_t* parent_dfs, const uint32_t* dfs2id,
                               const uint32_t* clade_id, const uint32_t* undefined_id, std::vector<uint32_t>& tab) {
    tab.assign((size_t)C * 2 * N, 0u);
    for (uint32_t c = 0; c < C; c++) {
        uint32_t* excl = tab.data() + (size_t)c * 2 * N;
        uint32_t* incl = excl + N;
        const uint32_t* own = clade_id + (size_t)c * N;
        for (uint32_t d = 0; d < N; d++) {
            excl[d] = d == 0 ? undefined_id[c] : incl[parent_dfs[d]];
            const uint32_t id = own[dfs2id[d]];
            incl[d] = id ? id : excl[d];
        }
    }
}

// what wepp_clade_assign requires of the pair CSR before anything goes to the device: 0, or the index of the first
// offending place + 1 in *where with a reason code (1 best_off[0] != 0, 2 offsets descend, 3 a node that is no BFS index)
inline int clade_check_pairs(uint32_t R, uint32_t N, const uint64_t* best_off, const uint32_t* best_nodes, uint64_t* where) {
    if (best_off[0] != 0) { *where = 0; return 1; }
    for (uint32_t r = 0; r < R; r++)
        if (best_off[r + 1] < best_off[r]) { *where = r; return 2; }
    for (uint64_t p = 0; p < best_off[R]; p++)
        if (best_nodes[p] >= N) { *where = p; return 3; }
    return 0;
}

}  // namespace wepp
