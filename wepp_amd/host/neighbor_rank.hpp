// neighbor_rank.hpp -- the host half of the neighbour sets: the reference's order of haplotypes (score_comparator,
// src/WEPP/arena.hpp:16-30), the ranking and truncation of a region (arena::closest_neighbors, arena.cpp:200-206;
// arena::highest_scoring_neighbors, :243-246) and the union over a selection ("add neighbors",
// src/WEPP/post_filter.hpp:56-64).  Haplotypes are arena indices into a table of keys; nothing here needs the device
// or the C-ABI library (tests/cxx/neighbors_host_sanitized.cpp runs it under the sanitizers).
#pragma once
#include <cmath>
#include <cstddef>
#include <set>
#include <string>
#include <vector>

static constexpr double SCORE_EPSILON = 1e-9;      // src/WEPP/config.hpp:15

struct haplotype_key {                              // what score_comparator reads of a haplotype
    double full_score = 0;                          // haplotype::full_score(): score * sqrt(dist_divergence)
    size_t leaf_count = 0;
    std::string id;
};

// arena.hpp:16-30: higher score first; within SCORE_EPSILON more leaves first, then the larger identifier.  A strict
// weak order when the scores are more than the epsilon apart or equal; chains of scores that are pairwise within it
// make the reference's own sets depend on their insertion order, and these too.
struct score_comparator {
    const std::vector<haplotype_key>* keys;
    bool operator()(int left, int right) const {
        const haplotype_key &l = (*keys)[(size_t)left], &r = (*keys)[(size_t)right];
        if (std::fabs(l.full_score - r.full_score) > SCORE_EPSILON) return l.full_score > r.full_score;
        if (l.leaf_count != r.leaf_count) return l.leaf_count > r.leaf_count;
        return l.id > r.id;
    }
};

// the first num_limit haplotypes of `region` in the comparator's order
inline std::vector<int> rank_neighbors(const std::vector<int>& region, const std::vector<haplotype_key>& keys, int num_limit) {
    std::set<int, score_comparator> all_neighbors(score_comparator{&keys});
    for (int h : region) all_neighbors.insert(h);
    std::vector<int> ret;
    for (int h : all_neighbors) {
        if ((int)ret.size() >= num_limit) break;
        ret.push_back(h);
    }
    return ret;
}

// the union of the ranked lists, in the comparator's order: the next round's input
inline std::vector<int> add_neighbors(const std::vector<std::vector<int>>& lists, const std::vector<haplotype_key>& keys) {
    std::set<int, score_comparator> build(score_comparator{&keys});
    for (const std::vector<int>& nbrs : lists) build.insert(nbrs.begin(), nbrs.end());
    return std::vector<int>(build.begin(), build.end());
}
