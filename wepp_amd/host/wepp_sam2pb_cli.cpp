// wepp_sam2pb_cli.cpp -- `wepp-sam2pb`: `wepp sam2PB` on files (sam_reader.hpp says what is computed and where it departs
// from the reference): SAM alignments + reference FASTA -> the merged reads .pb[.gz] that wepp-epp -r reads.
//   wepp-sam2pb -s in.sam[.gz] -f ref.fa -o reads.pb[.gz] [--min-af A] [--min-depth C] [--min-phred Q] [--max-reads M]
//               [--subsample-seed S [--subsample-trials T]] [--device N] [--dump DIR]
// Defaults 0.005, 10, 20, 1e9 (the reference's), T = 1000.  --dump DIR writes DIR/frequency_table.tsv: site, allele,
// frequency to 10 places, depth -- the raw table of all mapped reads, before the correction -- and, when reads were
// subsampled, DIR/subsample_trials.tsv: trial, divergence, chosen.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sam_reader.hpp"
#include "wepp_filter.hpp"

static const char USAGE[] =
    "usage: wepp-sam2pb -s in.sam[.gz] -f ref.fa -o reads.pb[.gz] [--min-af A] [--min-depth C] [--min-phred Q] [--max-reads M]\n"
    "                   [--subsample-seed S [--subsample-trials T]] [--device N] [--dump DIR]\n"
    "  SAM alignments -> merged reads (wepp sam2PB): bases below --min-phred (20) become N, alleles below --min-af (0.005) or at\n"
    "  sites below --min-depth (10) become N, equal reads merge.  --dump DIR writes DIR/frequency_table.tsv.\n"
    "  With --subsample-seed S, more than --max-reads (1e9) mapped reads are subsampled: of T (1000) seeded subsets of M reads the\n"
    "  one whose allele frequencies diverge least from the whole sample's is kept, the file is written from it, and --dump adds\n"
    "  DIR/subsample_trials.tsv (trial, divergence, chosen).  Equal seeds give equal files.\n"
    "  Unlike the reference: header and unmapped lines are skipped one by one; the earliest of equal reads names the merged\n"
    "  read; the subsample is a seeded hash order, not a shuffle seeded from the random device, and ties between trials go to\n"
    "  the lowest; without --subsample-seed more than --max-reads mapped reads is an error; malformed lines\n"
    "  (fewer than 11 fields, no quality, a CIGAR longer than the query, a read outside the reference) are errors naming the line.\n";

int main(int argc, char** argv) {
    std::string sam_f, ref_f, out_f, min_af_text = "0.005";
    sam2pb_options opt;
    for (int i = 1; i < argc; i++) {
        auto need = [&](const char* flag) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", flag); exit(1); }
            return argv[++i];
        };
        if (!strcmp(argv[i], "-s")) sam_f = need("-s");
        else if (!strcmp(argv[i], "-f")) ref_f = need("-f");
        else if (!strcmp(argv[i], "-o")) out_f = need("-o");
        else if (!strcmp(argv[i], "--min-af")) min_af_text = need("--min-af");
        else if (!strcmp(argv[i], "--min-depth")) opt.min_depth = atoi(need("--min-depth"));
        else if (!strcmp(argv[i], "--min-phred")) opt.min_phred = atoi(need("--min-phred"));
        else if (!strcmp(argv[i], "--max-reads")) opt.max_reads = atof(need("--max-reads"));
        else if (!strcmp(argv[i], "--subsample-seed")) { opt.subsample_seed = strtoull(need("--subsample-seed"), nullptr, 0); opt.subsample = true; }
        else if (!strcmp(argv[i], "--subsample-trials")) opt.subsample_trials = (uint32_t)strtoul(need("--subsample-trials"), nullptr, 10);
        else if (!strcmp(argv[i], "--device")) opt.device = atoi(need("--device"));
        else if (!strcmp(argv[i], "--dump")) opt.dump_dir = need("--dump");
        else { fputs(USAGE, stderr); return strcmp(argv[i], "--help") && strcmp(argv[i], "-h") ? 1 : 0; }
    }
    if (sam_f.empty() || ref_f.empty() || out_f.empty()) { fputs(USAGE, stderr); return 1; }
    try {
        opt.min_af = (double)std::stof(min_af_text);          // dataset::min_af is a float
    } catch (const std::exception&) {
        fprintf(stderr, "ERROR: --min-af '%s' is not a number\n", min_af_text.c_str());
        return 1;
    }
    try {
        const std::string reference = load_reference(ref_f);
        const sam2pb_stats st = sam2PB(sam_f, reference, out_f, opt);
        if (st.drawn)
            fprintf(stderr, "wepp-sam2pb: subsampled %zu of %zu mapped reads: trial %u of %u, divergence %.17g\n", st.kept, st.mapped, st.best_trial,
                    opt.subsample_trials, st.divergence);
        fprintf(stderr, "wepp-sam2pb: %zu mapped reads -> %zu merged reads (parse %.1f ms on the host, build %.1f ms)\n", st.mapped, st.merged,
                st.parse_ms, st.device_ms);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
