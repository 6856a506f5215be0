// sam_reader.hpp -- host-side mirror of `wepp sam2PB` (src/WEPP/sam2pb.cpp): the SAM parse of
// sam::add_reads (:157-258) on the host, and sam2PB itself (sam_reader.cpp parses, sam2pb.cpp runs sam::build through
// wepp_sam_build and writes the message of sam::dump_proto).  Same meaning of the arguments as the reference; errors
// throw MAT::mat_error.
//
// Departures from the reference, none of them silent:
//   - a header, empty or unmapped (FLAG bit 4) line is skipped; the reference's `return` at :167 drops the rest of the
//     TBB range the line happens to lie in;
//   - among equal reads the one earliest in the file leads the merged read and names it, and reverse_columns lists the
//     members in file order; the reference's unstable sort leaves both open;
//   - subsampling (:362-454) draws from std::random_device and has no defined result.  With a seed
//     (sam2pb_options::subsample) more mapped reads than max_reads are subsampled by wepp_sam_build_subsampled: the
//     draw is a seeded hash order instead of std::shuffle of a random_device-seeded mt19937, and among trials of equal
//     divergence the lowest wins (the reference's winner among equals depends on thread timing).  Without a seed more
//     mapped reads than max_reads is an error and nothing is written;
//   - inputs on which the reference reads outside its strings or tables are errors that name the line: fewer than 11
//     fields, a quality of `*` or shorter than the query, a CIGAR that consumes more bases than the query holds, an
//     aligned read that starts before position 1 or ends beyond the reference, a CIGAR without an aligned column;
//   - a '_' in the query becomes N (the reference's search in "ACGTN_" would keep it as a gap).
// Kept as the reference has it: the CIGAR's N advances the query index, and a chunk whose operator is no letter ('=')
// does not match the reference's \d+[A-Za-z] and is passed over.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "mat.hpp"

struct sam_aligned_read {                          // sam_read before the merge (sam2pb.hpp:14-18)
    std::string raw_name;
    int start_idx = 0;                             // 0-based site of the first column
    std::string aligned_string;                    // over ACGTN_
};

// One SAM line (:159-258): false when the line is skipped (empty, header, FLAG & 4).  `lineno` names the line in errors.
bool parse_sam_line(std::string const& line, size_t lineno, int min_phred, sam_aligned_read& out);
// Every mapped line of a SAM file (plain or .gz), in file order, handed to `sink` as it is read; reads that do not lie
// inside 1 .. genome_size are errors.  Returns the number of reads.
size_t parse_sam(std::string const& filename, size_t genome_size, int min_phred, std::function<void(sam_aligned_read&&)> const& sink);

struct sam2pb_options {                            // dataset::min_af / min_depth / min_phred / max_reads (defaults of main.cpp)
    double min_af = (double)0.005f;                // the option's text through std::stof, widened
    int min_depth = 10;
    int min_phred = 20;
    double max_reads = 1e9;
    int device = 0;
    std::string dump_dir;                          // non-empty: <dump_dir>/frequency_table.tsv in the layout of dump_sub_table (:30-52),
                                                   // and, when reads were drawn, <dump_dir>/subsample_trials.tsv: trial, divergence (%.17g), chosen
    bool subsample = false;                        // more mapped reads than max_reads: draw (true) or fail (false)
    uint64_t subsample_seed = 0;
    uint32_t subsample_trials = 1000;              // SUBSAMPLE_ITERS (config.hpp:6)
};
struct sam2pb_stats {
    size_t mapped = 0, merged = 0;
    double parse_ms = 0, device_ms = 0;
    bool drawn = false;                            // reads were subsampled: kept of mapped, the winning trial and its divergence
    size_t kept = 0; uint32_t best_trial = 0; double divergence = 0;
};
// sam2PB (:54-104): SAM + reference -> the reads .pb[.gz] of sam::dump_proto (:111-151)
sam2pb_stats sam2PB(std::string const& sam_filename, std::string const& reference, std::string const& pb_filename, sam2pb_options const& opt);
