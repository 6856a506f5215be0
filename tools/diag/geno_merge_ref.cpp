// geno_merge_ref.cpp -- the CPU baseline of tools/diag/geno_probe.py: the single-threaded merge of
// wepp_amd/host/haplotype_report.cpp (mutation_distance) over the pairs of the probe's groups.
//   geno_merge_ref input.bin max_pairs
// input.bin: u64 n_items, u64 n_groups, u64 item_off[n_items + 1], u32 grp_off[n_groups + 1], u32 item_word[]
// At most max_pairs pairs are measured (the first ones in the order i < j of each group); prints one JSON object with
// the pairs, the seconds and a checksum (the largest distance seen per group, summed) that keeps the loop alive.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../wepp_amd/host/haplotype_report.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: geno_merge_ref input.bin max_pairs\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    const unsigned long long max_pairs = strtoull(argv[2], nullptr, 10);
    uint64_t n_items = 0, n_groups = 0;
    if (fread(&n_items, 8, 1, f) != 1 || fread(&n_groups, 8, 1, f) != 1) return 1;
    std::vector<uint64_t> item_off(n_items + 1);
    std::vector<uint32_t> grp_off(n_groups + 1);
    if (fread(item_off.data(), 8, n_items + 1, f) != n_items + 1 || fread(grp_off.data(), 4, n_groups + 1, f) != n_groups + 1) return 1;
    std::vector<uint32_t> words(item_off[n_items]);
    if (fread(words.data(), 4, words.size(), f) != words.size()) return 1;
    fclose(f);
    std::vector<std::vector<MAT::Mutation>> geno(n_items);
    for (uint64_t i = 0; i < n_items; i++)
        for (uint64_t k = item_off[i]; k < item_off[i + 1]; k++) {
            MAT::Mutation m;
            m.position = (int)(words[k] & 0xFFFFF); m.ref_nuc = m.par_nuc = (int8_t)((words[k] >> 20) & 15); m.mut_nuc = (int8_t)((words[k] >> 24) & 15);
            geno[i].push_back(m);
        }
    unsigned long long pairs = 0, sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t g = 0; g < n_groups && pairs < max_pairs; g++) {
        int best = 0;
        for (uint32_t i = grp_off[g]; i < grp_off[g + 1] && pairs < max_pairs; i++)
            for (uint32_t j = i + 1; j < grp_off[g + 1] && pairs < max_pairs; j++, pairs++) {
                const int d = mutation_distance(geno[i], geno[j]);
                if (d > best) best = d;
            }
        sum += (unsigned long long)best;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"pairs\": %llu, \"seconds\": %.6f, \"pairs_per_s\": %.1f, \"checksum\": %llu}\n", pairs, s, s > 0 ? pairs / s : 0.0, sum);
    return 0;
}
