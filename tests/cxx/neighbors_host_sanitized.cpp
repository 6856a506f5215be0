// neighbors_host_sanitized.cpp -- the host-only code of the neighbour sets under AddressSanitizer + UBSan on the CPU
// (tests/test_neighbors_host_sanitized.py): score_comparator, the ranking and truncation of a region and the union over
// a selection (wepp_amd/host/neighbor_rank.hpp).
#include <algorithm>
#include <cstdio>
#include <random>

#include "../../wepp_amd/host/neighbor_rank.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    {
        // by hand: score first, then leaves, then the larger identifier; scores within the epsilon tie
        std::vector<haplotype_key> keys = {{1.0, 3, "a"}, {2.0, 1, "b"}, {1.0 + 1e-12, 5, "c"}, {1.0, 5, "d"}, {0.5, 9, "e"}, {2.0, 1, "bb"}};
        CHECK((rank_neighbors({0, 1, 2, 3, 4, 5}, keys, 500) == std::vector<int>{5, 1, 3, 2, 0, 4}));
        CHECK((rank_neighbors({4, 3, 2, 1, 0}, keys, 2) == std::vector<int>{1, 3}));
        CHECK((rank_neighbors({2}, keys, 1) == std::vector<int>{2}));
        CHECK(rank_neighbors({}, keys, 3).empty());
        CHECK((add_neighbors({{1, 3}, {}, {3, 4}, {5, 1}}, keys) == std::vector<int>{5, 1, 3, 4}));
        CHECK(add_neighbors({}, keys).empty());
        score_comparator cmp{&keys};
        CHECK(!cmp(2, 2) && cmp(3, 2) && !cmp(2, 3) && cmp(5, 1) && cmp(1, 0));
    }
    std::mt19937 rng(11);
    for (int round = 0; round < 200; round++) {
        // scores from a grid (equal or 0.25 apart), few leaf counts, distinct identifiers: a strict weak order
        const int n = 1 + (int)(rng() % 120);
        std::vector<haplotype_key> keys((size_t)n);
        for (int k = 0; k < n; k++) keys[(size_t)k] = haplotype_key{0.25 * (double)(rng() % 6), rng() % 3, "node_" + std::to_string(rng() % 7) + "_" + std::to_string(k)};
        std::vector<std::vector<int>> lists;
        std::vector<char> in_union((size_t)n, 0);
        for (int s = 0; s < 1 + (int)(rng() % 5); s++) {
            std::vector<int> region;
            for (int k = 0; k < n; k++)
                if (rng() % 3 == 0) region.push_back(k);
            std::shuffle(region.begin(), region.end(), rng);
            const int limit = 1 + (int)(rng() % 40);
            std::vector<int> want = region;
            std::sort(want.begin(), want.end(), score_comparator{&keys});
            if ((int)want.size() > limit) want.resize((size_t)limit);
            std::vector<int> got = rank_neighbors(region, keys, limit);
            CHECK(got == want);
            for (int h : got) in_union[(size_t)h] = 1;
            lists.push_back(got);
        }
        std::vector<int> want;
        for (int k = 0; k < n; k++)
            if (in_union[(size_t)k]) want.push_back(k);
        std::sort(want.begin(), want.end(), score_comparator{&keys});
        CHECK(add_neighbors(lists, keys) == want);
    }
    printf("ok\n");
    return 0;
}
