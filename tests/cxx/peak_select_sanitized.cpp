// peak_select_sanitized.cpp -- the choices of one step of the peak loop under AddressSanitizer + UBSan on the CPU
// (tests/test_peak_select_sanitized.py): the order of a tie group, the walk that accepts peaks and the stop rules
// (wepp_amd/host/peak_select.hpp), and one expansion round of wepp_filter::filter (expand_peaks, neighbor_rank.hpp).
// Distances come from a table here, from the device in wepp_epp_peaks.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../wepp_amd/host/neighbor_rank.hpp"
#include "../../wepp_amd/host/peak_select.hpp"

using namespace wepp;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {

using Places = std::vector<uint32_t>;

// haplotypes on a line: the distance between two is the difference of their coordinates
struct Line {
    std::vector<int> x;                 // by place in the group
    long long operator()(uint32_t old, uint32_t cand) const { return std::abs(x[old] - x[cand]); }
};

// the walk written the reference's way (every accepted one is asked, no early exit)
Places reference_walk(size_t n, uint32_t n_peaks, const PeakLimits& lim, const Line& d, size_t* reached) {
    Places acc;
    size_t i = 0;
    for (; i < n && acc.size() < lim.top_n && acc.size() + n_peaks < lim.max_peaks; i++) {
        bool valid = true;
        for (uint32_t old : acc)
            if (!(d(old, (uint32_t)i) > (long long)lim.peak_radius)) valid = false;
        if (valid) acc.push_back((uint32_t)i);
    }
    *reached = i;
    return acc;
}

}  // namespace

int main() {
    size_t reached = 0;
    {
        // far apart: everything is accepted until top_n.  Tie group smaller than, equal to and larger than top_n
        Line far{{0, 10, 20, 30, 40, 50}};
        CHECK((peak_consider(2, 0, PeakLimits{3, 300, 2}, far, &reached) == Places{0, 1}) && reached == 2);
        CHECK((peak_consider(3, 0, PeakLimits{3, 300, 2}, far, &reached) == Places{0, 1, 2}) && reached == 3);
        CHECK((peak_consider(6, 0, PeakLimits{3, 300, 2}, far, &reached) == Places{0, 1, 2}) && reached == 3);
        CHECK(peak_consider(0, 0, PeakLimits{3, 300, 2}, far, &reached).empty() && reached == 0);
        // the max_peaks cut in the middle of a group: 298 peaks exist, two more fit
        CHECK((peak_consider(6, 298, PeakLimits{10, 300, 2}, far, &reached) == Places{0, 1}) && reached == 2);
        CHECK(peak_consider(6, 300, PeakLimits{10, 300, 2}, far, &reached).empty() && reached == 0);
        CHECK((peak_consider(6, 0, PeakLimits{10, 1, 2}, far) == Places{0}));
    }
    {
        // all candidates rejected but the first: everything within the radius of place 0; the walk reaches the end
        Line near{{5, 6, 7, 4, 3, 5}};
        CHECK((peak_consider(6, 0, PeakLimits{10, 300, 2}, near, &reached) == Places{0}) && reached == 6);
        // radius 0 accepts everything that is not at distance 0
        CHECK((peak_consider(6, 0, PeakLimits{10, 300, 0}, near) == Places{0, 1, 2, 3, 4}));
        // a rejected candidate does not object to later ones: 1 is within 2 of 0, 3 is 3 from 0 and 1 from the rejected 2
        Line chain{{0, 2, 4, 3}};
        CHECK((peak_consider(4, 0, PeakLimits{10, 300, 2}, chain) == Places{0, 2}));
    }
    {
        // the order of a group: rank ascending, arena index among equal ranks, arena index alone without ranks
        const uint32_t rank[8] = {5, 1, 3, 1, 9, 3, 0, 1};
        std::vector<uint32_t> g = {7, 4, 1, 6, 3, 0, 5, 2};
        std::vector<double> carry = {70, 40, 10, 60, 30, 0, 50, 20};
        peak_order_group(g, rank, &carry);
        CHECK((g == Places{6, 1, 3, 7, 2, 5, 0, 4}));
        CHECK((carry == std::vector<double>{60, 10, 30, 70, 20, 50, 0, 40}));
        g = {7, 4, 1, 6};
        peak_order_group(g, nullptr);
        CHECK((g == Places{1, 4, 6, 7}));
        const uint32_t same[8] = {2, 2, 2, 2, 2, 2, 2, 2};          // equal ranks
        g = {5, 0, 3};
        peak_order_group(g, same);
        CHECK((g == Places{0, 3, 5}));
        g.clear();
        peak_order_group(g, rank, &carry);                          // (an empty group; a carry of another size is left alone)
        CHECK(g.empty() && carry.size() == 8);
    }
    // the stop rules
    CHECK(peak_no_leader(0, 1.0, 1e-9) && peak_no_leader(3, 0.5e-9, 1e-9) && !peak_no_leader(3, 1e-9, 1e-9));
    CHECK(peak_done(300, 300, 5) && peak_done(2, 300, 0) && !peak_done(299, 300, 1));

    {
        // an expansion round: peaks in ascending arena index whatever their order, regions ranked by score, peaks and
        // the round's earlier neighbours passed over, the cut per peak counting only what was taken
        std::vector<haplotype_key> keys = {{5.0, 1, "a"}, {4.0, 1, "b"}, {3.0, 1, "c"}, {2.0, 1, "d"}, {1.0, 1, "e"}, {0.5, 1, "f"}, {0.25, 1, "g"}};
        // peak 4 (listed first) and peak 0; 0 is served first and takes the two best that are no peaks: 1, 2
        CHECK((expand_peaks({4, 0}, {{4, 1, 2, 3, 5}, {0, 1, 2, 3, 4}}, keys, 2) == std::vector<int>{1, 2, 3, 5}));
        CHECK((expand_peaks({4, 0}, {{4, 1, 2, 3, 5}, {0, 1, 2, 3, 4}}, keys, 1) == std::vector<int>{1, 2}));
        CHECK((expand_peaks({0, 4}, {{0, 1, 2, 3, 4}, {4, 1, 2, 3, 5}}, keys, 50) == std::vector<int>{1, 2, 3, 5}));
        CHECK(expand_peaks({0}, {{0}}, keys, 50).empty() && expand_peaks({}, {}, keys, 50).empty());
        CHECK(expand_peaks({6}, {{}}, keys, 50).empty());
    }
    std::mt19937 rng(7);
    for (int round = 0; round < 2000; round++) {
        const size_t n = rng() % 40;
        Line d;
        for (size_t i = 0; i < n; i++) d.x.push_back((int)(rng() % 30));
        const PeakLimits lim{1 + (uint32_t)(rng() % 12), 1 + (uint32_t)(rng() % 20), (uint32_t)(rng() % 4)};
        const uint32_t n_peaks = (uint32_t)(rng() % (lim.max_peaks + 2));
        size_t want_reached = 0;
        const Places want = reference_walk(n, n_peaks, lim, d, &want_reached);
        // the callback is only ever asked about an accepted place and a later candidate, accepted ones in order
        uint32_t last_old = 0;
        uint32_t last_cand = 0;
        bool in_order = true;
        const Places got = peak_consider(n, n_peaks, lim, [&](uint32_t old, uint32_t cand) {
            if (old >= cand || cand >= n) in_order = false;
            if (cand == last_cand && old < last_old) in_order = false;
            last_old = old; last_cand = cand;
            return d(old, cand);
        }, &reached);
        CHECK(got == want && reached == want_reached && in_order);
        CHECK(got.size() <= lim.top_n && (got.empty() || got.size() + n_peaks <= lim.max_peaks));
    }
    printf("ok\n");
    return 0;
}
