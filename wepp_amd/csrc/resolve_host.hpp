// resolve_host.hpp -- the parts of wepp_epp_resolve's host side that need no device: the checks on the
// residual list and its order by position (resolve_capi.cpp; a plain C++ program can include this alone).
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/wepp_place.h"
#include "errors.hpp"

namespace wepp {

// WEPP_OK, or WEPP_EINVAL with the message set
inline int resolve_check_residual(uint32_t n_res, const uint32_t* res_word, uint32_t genome_size) {
    for (uint32_t m = 0; m < n_res; m++) {
        const uint32_t w = res_word[m], pos = w & 0xFFFFFu, ref = (w >> 20) & 15u, mut = (w >> 24) & 15u;
        const std::string who = "residual mutation " + std::to_string(m);
        if (pos < 1 || pos > genome_size)
            return set_error(WEPP_EINVAL, who + ": position " + std::to_string(pos) + " is outside 1 .. genome_size");
        if (mut == 0 || mut == 15) return set_error(WEPP_EINVAL, who + ": mut_nuc must be an allele mask 1 .. 14");
        if (ref == 0 || (ref & (ref - 1))) return set_error(WEPP_EINVAL, who + ": ref_nuc must be a one-hot mask");
    }
    return WEPP_OK;
}

// by position, stably: the caller's order survives within a position (two residual mutations at one position
// act on a read in that order).  idx[i] = place in the caller's list of the i-th of the sorted one.
inline void resolve_sort_residual(uint32_t n_res, const uint32_t* res_word, std::vector<uint32_t>& pos,
                                  std::vector<uint32_t>& word, std::vector<uint32_t>& idx) {
    idx.resize(n_res);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(),
                     [&](uint32_t a, uint32_t b) { return (res_word[a] & 0xFFFFFu) < (res_word[b] & 0xFFFFFu); });
    pos.resize(n_res);
    word.resize(n_res);
    for (uint32_t i = 0; i < n_res; i++) {
        word[i] = res_word[idx[i]];
        pos[i] = word[i] & 0xFFFFFu;
    }
}

}  // namespace wepp
