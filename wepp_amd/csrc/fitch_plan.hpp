// fitch_plan.hpp -- what a Fitch-Sankoff run decides on the host (fitch_capi.cpp): the form of the kernels, the chunk
// and level tables of the tree, the shape of the run.  Functions of plain arrays and values: no HIP call and no getenv
// (fitch.hpp names HIP's types); a test hook arrives as a value, negative when it is not set.
// tests/cxx/fitch_plan_main.cpp runs them without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wepp_place.h"
#include "errors.hpp"
#include "fitch.hpp"

namespace wepp {

// levels: the level-synchronous kernels; else one of the two stack forms, sets (sets_ok) or scores
struct FitchForm { bool levels, sets_ok; };

// The set forms need non-empty allele sets and a tree within their counters (sets_ok_tree); the level form is the set
// form of choice.  force_scores / force_dfs: the test hooks WEPP_FITCH_SCORES=1 / WEPP_FITCH_DFS=1.
// only the stack forms have a stack: the level form takes a tree of any depth (one launch pair per level)
inline int fitch_choose_form(bool sets_ok_tree, bool force_scores, bool force_dfs, bool empty_set, uint32_t max_depth, FitchForm* out) {
    const bool sets_ok = sets_ok_tree && !force_scores && !empty_set;
    const bool levels = sets_ok && !force_dfs;
    if (!levels && max_depth > FITCH_MAX_DEPTH)
        return set_error(WEPP_ELIMIT, "tree depth " + std::to_string(max_depth) + " exceeds the LDS stack (" +
                                          std::to_string(FITCH_MAX_DEPTH) + ") of the form these rows need");
    *out = FitchForm{levels, sets_ok};
    return WEPP_OK;
}

// chunks of consecutive DFS nodes (one wave each) and what is open at their boundaries: only the two stack forms
// use them
struct FitchChunks {
    uint32_t D = 0, C = 0;                      // rows of `open` per chunk (max_depth + 1), chunks
    std::vector<uint32_t> start, depth, min, open;      // FitchTree's chunk_start, chunk_depth, chunk_min, chunk_open
};

// hook: the number of chunks forced by WEPP_FITCH_CHUNKS, clamped to [1, N]
inline FitchChunks fitch_build_chunks(uint32_t N, long hook, uint32_t max_depth, const uint32_t* parent_dfs, const uint32_t* depth) {
    FitchChunks t;
    const uint32_t D = t.D = max_depth + 1;
    uint32_t C = std::max<uint32_t>(1, std::min<uint32_t>(256, N / 2048));
    if (hook >= 0) C = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)hook, N));
    t.C = C;
    t.start.assign(C + 1, 0); t.depth.assign(C + 1, 0); t.min.assign(C, 0); t.open.assign((size_t)(C + 1) * D, 0);
    for (uint32_t c = 0; c <= C; c++) t.start[c] = (uint32_t)((uint64_t)N * c / C);
    for (uint32_t c = 0; c <= C; c++) {
        // nodes open before node a (c < C): its strict ancestors; after the last node: the
        // strict ancestors of that leaf (the single node itself when the tree is one node)
        uint32_t x;
        if (c < C) { x = t.start[c]; t.depth[c] = depth[x]; }
        else if (N == 1) { t.depth[c] = 1; t.open[(size_t)c * D] = 0; continue; }
        else { x = N - 1; t.depth[c] = depth[x]; }
        uint32_t anc = x;
        for (uint32_t k = t.depth[c]; k-- > 0;) {
            anc = parent_dfs[anc];
            t.open[(size_t)c * D + k] = anc;
        }
    }
    for (uint32_t c = 0; c < C; c++) {
        uint32_t mn = 0xFFFFFFFFu;
        for (uint32_t d = t.start[c]; d < t.start[c + 1]; d++) mn = std::min(mn, depth[d]);
        t.min[c] = mn;
    }
    return t;
}

// level-synchronous form: the topology in BFS order (levels and sibling groups are contiguous)
struct FitchLevelTables {
    std::vector<uint32_t> level_off;            // [levels + 1] first BFS index of every level, then N
    std::vector<uint32_t> coff, par;            // FitchLevels' coff [N + 1] and parent [N]
};

inline FitchLevelTables fitch_build_levels(uint32_t N, const uint32_t* parent_dfs, const uint32_t* depth, const uint32_t* dfs2bfs) {
    FitchLevelTables t;
    std::vector<uint32_t> bfs2dfs(N);
    for (uint32_t d = 0; d < N; d++) bfs2dfs[dfs2bfs[d]] = d;
    t.coff.assign((size_t)N + 1, 0); t.par.assign(N, 0);
    for (uint32_t bidx = 0; bidx < N; bidx++) {
        const uint32_t d = bfs2dfs[bidx];
        if (bidx == 0 || depth[d] != depth[bfs2dfs[bidx - 1]]) t.level_off.push_back(bidx);
        if (d == 0) continue;
        const uint32_t pb = dfs2bfs[parent_dfs[d]];
        t.par[bidx] = pb;
        t.coff[pb + 1]++;                              // BFS visits a node's children consecutively, parents in order
    }
    t.coff[0] = 1;                                     // the first child (if any) is BFS node 1
    for (uint32_t i = 0; i < N; i++) t.coff[i + 1] += t.coff[i];
    t.level_off.push_back(N);
    return t;
}

// A run's rows go in batches (64 rows, 64 * FITCH_ROWS_PER_LANE for the level form) and the batches in groups that
// share one launch: as many as fit half of what the device has free.
struct FitchShape {
    uint32_t rows_per_batch, nbatches, group;
    size_t part_bytes;                          // of one batch's partial-sum scratch array (there are two)
    size_t tables_need;                         // bytes of the decision tables of a group
};

// free_b: free device memory; tables_bytes: the decision tables the plan already holds -- part of what a run may use
// (without them in the sum every run after the first saw half the memory and cut its rows into twice as many groups).
// hook: WEPP_FITCH_GROUP, at most this many batches per group.
inline FitchShape fitch_run_shape(uint32_t N, uint32_t n_sites, bool levels, uint32_t C, uint32_t D, size_t free_b, size_t tables_bytes, long hook) {
    FitchShape s;
    s.rows_per_batch = levels ? 64 * FITCH_ROWS_PER_LANE : 64;
    s.nbatches = (n_sites + s.rows_per_batch - 1) / s.rows_per_batch;
    // per batch: the decision tables and the two partial-sum scratch arrays
    s.part_bytes = levels ? 0 : (size_t)C * D * 64 * 16;
    const size_t per_batch = (size_t)N * s.rows_per_batch + 2 * s.part_bytes;
    const size_t budget = (free_b + tables_bytes) / 2;
    s.group = (uint32_t)std::max<size_t>(1, std::min<size_t>(s.nbatches, budget / std::max<size_t>(per_batch, 1)));
    if (hook >= 0) s.group = std::max<uint32_t>(1, std::min<uint32_t>(s.group, (uint32_t)hook));
    s.tables_need = (size_t)N * s.rows_per_batch * s.group;
    return s;
}

}  // namespace wepp
