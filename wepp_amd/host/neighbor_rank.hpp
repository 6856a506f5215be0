// neighbor_rank.hpp -- the host half of the neighbour sets: the reference's order of haplotypes (score_comparator,
// src/WEPP/arena.hpp:16-30), the ranking and truncation of a region (arena::closest_neighbors, arena.cpp:200-206;
// arena::highest_scoring_neighbors, :243-246) and the union over a selection ("add neighbors",
// src/WEPP/post_filter.hpp:56-64).  Haplotypes are arena indices into a table of keys; nothing here needs the device
// or the C-ABI library (tests/cxx/neighbors_host_sanitized.cpp runs it under the sanitizers).  expand_peaks is one
// expansion round of wepp_filter::filter (src/WEPP/initial_filter.cpp:474-497).
#pragma once
#include <algorithm>
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

// One expansion round of wepp_filter::filter (initial_filter.cpp:475-497): the peaks are taken in ascending arena index
// (the reference walks a std::set of pointers into the arena); regions[j] is the highest_scoring_neighbors region of
// peaks[j] at the round's radius; of each region, in the comparator's order over `keys` (the ORIGINAL scores:
// recover_haplotype_state, :476), the haplotypes that are neither a peak nor a neighbour of this round yet are taken, at
// most max_neighbors per peak.  Returns the round's neighbours, ascending.
inline std::vector<int> expand_peaks(const std::vector<int>& peaks, const std::vector<std::vector<int>>& regions,
                                     const std::vector<haplotype_key>& keys, int max_neighbors) {
    std::vector<size_t> order(peaks.size());
    for (size_t j = 0; j < order.size(); j++) order[j] = j;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return peaks[a] < peaks[b]; });
    const std::set<int> is_peak(peaks.begin(), peaks.end());
    std::set<int> curr_neighbors;
    for (size_t j : order) {
        int i = 0;
        for (int node : rank_neighbors(regions[j], keys, (int)regions[j].size())) {
            if (is_peak.count(node) || curr_neighbors.count(node)) continue;
            curr_neighbors.insert(node);
            if (++i == max_neighbors) break;
        }
    }
    return std::vector<int>(curr_neighbors.begin(), curr_neighbors.end());
}
