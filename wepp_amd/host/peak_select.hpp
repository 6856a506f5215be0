// peak_select.hpp -- the choices of one step of wepp_filter's peak loop (wepp_filter::step,
// src/WEPP/initial_filter.cpp:387-453) as plain C++: the order of a tie group, the walk over it that accepts peaks, and
// the stop rules.  No device, no I/O: wepp_epp_peaks (wepp_amd/csrc/peaks_capi.cpp) supplies the tie group, the ranks
// and the distances; tests/cxx/peak_select_sanitized.cpp runs it alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace wepp {

struct PeakLimits {
    uint32_t top_n, max_peaks, peak_radius;
};

// The place score_comparator (arena.hpp:16-31) gives haplotypes whose full scores tie: tie_rank ascending (the caller
// derives it from leaf_count and id), lower arena index first among equal ranks and when there are no ranks.
// `carry` (may be null) is permuted along with the group.
inline void peak_order_group(std::vector<uint32_t>& group, const uint32_t* tie_rank, std::vector<double>* carry = nullptr) {
    std::vector<uint32_t> idx(group.size());
    for (uint32_t i = 0; i < idx.size(); i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        const uint32_t ga = group[a], gb = group[b];
        if (tie_rank && tie_rank[ga] != tie_rank[gb]) return tie_rank[ga] < tie_rank[gb];
        return ga < gb;
    });
    std::vector<uint32_t> g(group.size());
    for (uint32_t i = 0; i < idx.size(); i++) g[i] = group[idx[i]];
    group.swap(g);
    if (carry && carry->size() == idx.size()) {
        std::vector<double> c(idx.size());
        for (uint32_t i = 0; i < idx.size(); i++) c[i] = (*carry)[idx[i]];
        carry->swap(c);
    }
}

// The walk of :410-432 over an ordered tie group: a candidate is looked at while fewer than top_n are accepted and
// accepted + n_peaks < max_peaks, and accepted iff dist(old, i) > peak_radius for every accepted place `old`, where
// dist(old, i) is group[old]->mutation_distance(group[i]) (valid_two_tops, initial_filter.hpp:47-49).  The accepted
// are asked in the order they were accepted, so a caller that computes an accepted peak's distances when they are first
// wanted computes them in that order.  Returns the places in `group` of the accepted, in order; *looked_at (may be
// null) receives how many candidates the walk reached.
template <typename Dist>
inline std::vector<uint32_t> peak_consider(size_t group_size, uint32_t n_peaks, const PeakLimits& lim, Dist&& dist, size_t* looked_at = nullptr) {
    std::vector<uint32_t> accepted;
    size_t i = 0;
    for (; i < group_size && accepted.size() < lim.top_n && accepted.size() + n_peaks < lim.max_peaks; i++) {
        bool valid = true;
        for (uint32_t k = 0; k < accepted.size(); k++)      // (the reference asks every one, we stop at the first that objects)
            if ((long long)dist(accepted[k], (uint32_t)i) <= (long long)lim.peak_radius) { valid = false; break; }
        if (valid) accepted.push_back((uint32_t)i);
    }
    if (looked_at) *looked_at = i;
    return accepted;
}

// :400 -- no leader: nothing is live, or the largest full score is below eps
inline bool peak_no_leader(uint32_t n_live, double m, double eps) { return n_live == 0 || m < eps; }
// :452, behind a step (an empty `current` is the next step's peak_no_leader)
inline bool peak_done(uint32_t n_peaks, uint32_t max_peaks, uint32_t n_remaining) { return n_peaks >= max_peaks || n_remaining == 0; }

}  // namespace wepp
