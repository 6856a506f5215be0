// sam2pb.cpp -- sam2PB of sam_reader.hpp: the parse on the host, sam::build on the device (wepp_sam_build, or
// wepp_sam_build_subsampled when a seed is given and more reads are mapped than max_reads), and the message of
// sam::dump_proto (src/WEPP/sam2pb.cpp:54-151) over the reads that were kept.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>

#include "../../include/wepp_place.h"
#include "sam_reader.hpp"
#include "wepp_filter.hpp"

using MAT::mat_error;

namespace {

const char GENOME_STRING[] = "ACGTN_";             // sam2pb.hpp:10

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// dump_sub_table (:30-52): per site the alleles seen, most frequent first
void dump_frequency_table(std::vector<int32_t> const& freq, size_t genome_size, std::string const& name) {
    FILE* f = fopen(name.c_str(), "w");
    if (!f) throw mat_error("ERROR: Could not write " + name);
    fprintf(f, "Position\tAllele\tFrequency\tDepth\n");
    for (size_t i = 0; i < genome_size; i++) {
        int sum = 0;
        std::vector<std::pair<int, int>> res;
        for (int j = 0; j < 6; j++) {
            sum += freq[i * 6 + j];
            if (freq[i * 6 + j]) res.emplace_back(freq[i * 6 + j], j);
        }
        std::sort(res.begin(), res.end(), std::greater<>());
        for (auto const& cj : res) fprintf(f, "%zu\t%c\t%.10f\t%d\n", i + 1, GENOME_STRING[cj.second], (double)cj.first / sum, sum);
    }
    fclose(f);
}

}  // namespace

sam2pb_stats sam2PB(std::string const& sam_filename, std::string const& reference, std::string const& pb_filename, sam2pb_options const& opt) {
    sam2pb_stats stats;
    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::string> names;
    std::vector<uint32_t> start;
    std::vector<uint64_t> base_off{0};
    std::vector<uint8_t> base;
    stats.mapped = parse_sam(sam_filename, reference.size(), opt.min_phred, [&](sam_aligned_read&& rd) {
        if (!opt.subsample && (double)(names.size() + 1) > opt.max_reads)
            throw mat_error("ERROR: more than --max-reads (" + std::to_string((long long)opt.max_reads) + ") mapped reads: the reference would subsample them at random (sam2pb.cpp:362-454), which has no defined result; nothing was written");
        names.push_back(std::move(rd.raw_name));
        start.push_back((uint32_t)rd.start_idx);
        for (char c : rd.aligned_string) base.push_back((uint8_t)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : c == 'N' ? 4 : 5));
        base_off.push_back(base.size());
    });
    stats.parse_ms = ms_since(t0);
    if (names.empty()) throw mat_error("Zero reads; likely did not find input sam file");      // :332-335

    t0 = std::chrono::steady_clock::now();
    const uint32_t R = (uint32_t)names.size();
    const size_t G = reference.size();
    std::vector<int32_t> freq(opt.dump_dir.empty() ? 0 : G * 6);
    std::vector<uint32_t> order(R), group_off((size_t)R + 1), read_off((size_t)R + 1), words;
    std::vector<int32_t> m_start(R), m_end(R), m_degree(R);
    uint32_t M = 0;
    wepp_sam_reads rd{R, start.data(), base_off.data(), base.data()};
    wepp_sam_params par{opt.min_af, (uint32_t)std::max(opt.min_depth, 0)};
    wepp_sam_out out{};
    out.freq = freq.empty() ? nullptr : freq.data();
    out.n_merged = &M; out.order = order.data(); out.group_off = group_off.data(); out.read_off = read_off.data();
    out.start = m_start.data(); out.end = m_end.data(); out.degree = m_degree.data();
    out.read_word = nullptr; out.word_capacity = 0;          // the words' number is the call's to tell: they are fetched
    // more mapped reads than max_reads, and a seed: sam::subsample (:362-454) through the library's defined draw
    const bool draw = opt.subsample && (double)R > opt.max_reads;
    std::vector<uint32_t> kept;
    std::vector<double> divergence;
    uint32_t n_kept = 0, best_trial = 0;
    int rc;
    if (draw) {
        const wepp_sam_subsample_params sub{opt.subsample_seed, opt.max_reads < 1 ? 0u : (uint32_t)opt.max_reads, opt.subsample_trials};
        kept.resize(std::max<uint32_t>(sub.max_reads, 1));
        divergence.resize(std::max<uint32_t>(sub.trials, 1));
        wepp_sam_subsample_out so{&n_kept, kept.data(), &best_trial, divergence.data(), nullptr};
        rc = wepp_sam_build_subsampled(opt.device, (const uint8_t*)reference.data(), (uint32_t)G, &rd, &par, &sub, &out, &so);
    } else {
        rc = wepp_sam_build(opt.device, (const uint8_t*)reference.data(), (uint32_t)G, &rd, &par, &out);
    }
    if (rc == WEPP_ELIMIT && M && read_off[M] > 0) {
        words.resize(read_off[M]);
        rc = wepp_sam_fetch_words(words.data(), words.size());
    }
    if (rc != WEPP_OK) throw mat_error(std::string(draw ? "wepp_sam_build_subsampled: " : "wepp_sam_build: ") + wepp_last_error());
    if (draw) {
        stats.drawn = true; stats.kept = n_kept; stats.best_trial = best_trial; stats.divergence = divergence[best_trial];
    }
    stats.device_ms = ms_since(t0);
    stats.merged = M;

    // the merged reads as sam::dump_proto writes them: the content is the reference under the read's words
    std::vector<sam_read_record> records(M);
    std::map<std::string, std::vector<std::string>> reverse_merge;
    for (uint32_t g = 0; g < M; g++) {
        sam_read_record& r = records[g];
        r.start_idx = m_start[g];
        r.degree = m_degree[g];
        r.content = reference.substr((size_t)m_start[g] - 1, (size_t)(m_end[g] - m_start[g] + 1));
        for (uint32_t k = read_off[g]; k < read_off[g + 1]; k++) {
            const uint32_t pos = words[k] & 0xFFFFFu, mut = (words[k] >> 24) & 15u;
            r.content[pos - (uint32_t)m_start[g]] = mut == 1 ? 'A' : mut == 2 ? 'C' : mut == 4 ? 'G' : mut == 8 ? 'T' : 'N';
        }
        // sam_read::degree_name (sam2pb.hpp:20-25) of the group's leader
        r.name = names[order[group_off[g]]] + "_READ_" + std::to_string(m_start[g]) + "_" + std::to_string(m_end[g]) + "_" + std::to_string(m_degree[g]);
        std::vector<std::string>& members = reverse_merge[r.name];                             // :348-357
        for (uint32_t s = group_off[g]; s < group_off[g + 1]; s++) members.push_back(names[order[s]]);
    }
    dump_reads_proto(records, reverse_merge, pb_filename);
    if (!opt.dump_dir.empty()) dump_frequency_table(freq, G, opt.dump_dir + "/frequency_table.tsv");
    if (!opt.dump_dir.empty() && draw) {
        const std::string name = opt.dump_dir + "/subsample_trials.tsv";
        FILE* f = fopen(name.c_str(), "w");
        if (!f) throw mat_error("ERROR: Could not write " + name);
        fprintf(f, "trial\tdivergence\tchosen\n");
        for (uint32_t t = 0; t < opt.subsample_trials; t++) fprintf(f, "%u\t%.17g\t%d\n", t, divergence[t], t == best_trial ? 1 : 0);
        fclose(f);
    }
    return stats;
}
