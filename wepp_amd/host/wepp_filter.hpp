// wepp_filter.hpp -- host-side mirror of the slice of WEPP's own interface that feeds and
// consumes wepp_filter::cartesian_map (/root/reference/src/WEPP/): raw_read, the reads .pb
// loader, read masking, the condensed tree, the call itself on top of wepp_epp_map, the
// read loop of arena::dump_read2haplotype_mapping on top of wepp_epp_assign,
// arena::resolve_unaccounted_mutations on top of wepp_epp_resolve, and arena::closest_neighbors with the
// "add neighbors" step of post_filter::iterative_filter on top of wepp_epp_neighbors, and wepp_filter::filter itself:
// the peak loop on top of wepp_epp_peaks and the five expansion rounds on top of wepp_epp_neighbors.
// Same names and argument meaning as the reference; errors throw MAT::mat_error.
#pragma once
#include <array>
#include <map>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "mat.hpp"
#include "neighbor_rank.hpp"
#include "residual_file.hpp"

static constexpr int NUM_RANGE_BINS = 50;          // src/WEPP/config.hpp:13
static constexpr int MAX_CACHED_EPP_SIZE = 2048;   // src/WEPP/config.hpp:9

struct raw_read {                                   // src/WEPP/read.hpp:8-14
    std::string read;
    std::vector<MAT::Mutation> mutations;
    int start = 0;
    int end = 0;
    int degree = 0;
};

// FASTA -> upper-cased sequence without the header line (dataset.hpp:179-203)
std::string load_reference(std::string const& fasta_filename);
// third column of every line of mask.bed; a missing file means no mask (dataset.hpp:90-113)
std::vector<int> load_masked_sites(std::string const& bed_filename);

// sam.proto message `sam` -> raw_reads (sam2pb.cpp:489-549): start = start_idx (1-based),
// end = start + len(content) - 1, one mutation wherever content differs from the reference and
// is not '_'; 'N' is missing.  reverse_merge receives the column merge table (:539-545).
std::vector<raw_read> load_reads_from_proto(std::string const& reference, std::string const& filename,
                                            std::unordered_map<std::string, std::vector<std::string>>& reverse_merge);
// the writer side of the same message (sam::dump_proto, sam2pb.cpp:111-147), for fixtures:
// reads given as (name, 1-based start, aligned content over ACGTN_, degree)
struct sam_read_record { std::string name; int start_idx; std::string content; int degree; };
void dump_reads_proto(std::vector<sam_read_record> const& reads, std::string const& filename);
// ... with the reverse_columns table behind the reads (:122-129: one column_info per entry of reverse_merge, in the
// order of its keys), gzip-compressed when the name holds ".gz" (:136)
void dump_reads_proto(std::vector<sam_read_record> const& reads, std::map<std::string, std::vector<std::string>> const& reverse_merge,
                      std::string const& filename);

// arena::arena, arena.hpp:58-72: mutations at masked sites are removed from the reads
void mask_reads(std::vector<raw_read>& reads, std::vector<int> const& masked_sites);
// arena::site_read_map, arena.hpp:157-175: sites covered by a non-N, non-masked read base
std::unordered_set<int> site_read_map(std::vector<raw_read> const& reads, std::vector<int> const& masked_sites);
// util.cpp:79-133: keeps the mutations at covered sites; a node left without mutations is
// merged into its nearest kept ancestor (node_mappings: condensed node -> original nodes)
MAT::Tree create_condensed_tree(MAT::Node* ref_root, const std::unordered_set<int>& site_read_map,
                                std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings);

// what wepp_filter::cartesian_map leaves behind (initial_filter.cpp:140-239, without the final
// sort): haplotypes in arena order = pre-order of the condensed tree (arena.cpp:3-55)
struct cartesian_map_result {
    std::vector<MAT::Node*> haplotypes;                          // condensed_source of haplotype k
    std::vector<double> score, dist_divergence;                  // haplotype::score (= orig_score), ::dist_divergence
    std::vector<std::array<int, NUM_RANGE_BINS>> mapped_read_counts;
    std::vector<int> max_parismony, parsimony_multiplicity;      // per read (:203-204)
    std::vector<std::vector<int>> epp_positions_cache;           // per read: arena indices, sorted (:205-210)
};
// returns 0, or 1 after printing the error (the reference's convention for this layer)
int cartesian_map(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                  cartesian_map_result& out, int device = 0);

// what the read loop of arena::dump_read2haplotype_mapping computes (arena.cpp:610-667), per SELECTED haplotype, in
// the order of `selected` (the reference's `abundance` order): the reads whose set of nearest selected haplotypes
// (haplotype::mutation_distance, haplotype.hpp:123-177) holds it, as ascending indices into `reads`, the sum of
// their degree (the count of :859-865), and the fraction of the genome they cover (:637-665, :683-684)
struct read2haplotype_result {
    std::vector<int> min_dist;                                   // per read: distance to its nearest selected haplotypes
    std::vector<std::vector<int>> reads;                         // per selected haplotype
    std::vector<long long> degree;
    std::vector<double> coverage;
};
// `selected`: nodes of `condensed`, distinct.  Returns 0, or 1 after printing the error.
int read2haplotype_mapping(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                           const std::vector<MAT::Node*>& selected, read2haplotype_result& out, int device = 0);

// residual_mutations.txt (arena.cpp:708-731) -> the residual mutations in the order of the file; throws
// MAT::mat_error (residual_file.hpp lists what is refused)
std::vector<residual_mutation> load_residual_mutations(std::string const& filename, std::string const& reference);

// what arena::resolve_unaccounted_mutations computes (arena.cpp:739-892), per residual mutation, in the order of
// `residual`: the reads that carry it (ascending indices into `reads`; the rows of mutation_reads.csv), how many reads
// hold an N at its site, and the selected haplotypes its reads point to (indices into `selected`, ascending: those
// among the haplotypes nearest to some covered or masked read whose summed degree is the largest; the rows of
// mutation_haplotypes.csv)
struct resolve_result {
    std::vector<std::vector<int>> covered_reads;
    std::vector<size_t> n_masked;
    std::vector<std::vector<int>> best;
    std::vector<long long> best_degree;
};
// `selected`: nodes of `condensed`, distinct.  Returns 0, or 1 after printing the error.
int resolve_unaccounted_mutations(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                                  const std::vector<MAT::Node*>& selected, const std::vector<residual_mutation>& residual,
                                  resolve_result& out, int device = 0);

// haplotype::leaf_count (arena.cpp:16, get_num_leaves, util.cpp:298-316) of every haplotype of `haplotypes`: the
// leaves of the uncondensed tree below the first node its condensed node stands for
std::vector<size_t> haplotype_leaf_counts(const std::vector<MAT::Node*>& haplotypes,
                                          const std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings);
// what score_comparator reads, per haplotype of a finished map (arena order): full_score, leaf_count, identifier
std::vector<haplotype_key> haplotype_keys(const cartesian_map_result& map, const std::vector<size_t>& leaf_count);

// arena::closest_neighbors (arena.cpp:171-207) for every haplotype of `selected` in one device call: all haplotypes
// within max_radius mutations of it (node->mutation_distance(target)) that are reached through haplotypes within the
// radius, the num_limit best of them in score_comparator's order -- arena indices, i.e. indices into `keys` -- with
// their distances; next_selection: the union over the selection in the same order (post_filter.hpp:56-64)
struct neighbors_result {
    std::vector<std::vector<int>> neighbors, distance;            // per selected haplotype, rank order
    std::vector<int> next_selection;
};
// `selected`: nodes of `condensed`, distinct; `keys`: haplotype_keys of the map over `condensed`.  Returns 0, or 1
// after printing the error.
int closest_neighbors(MAT::Tree& condensed, const std::vector<MAT::Node*>& selected, const std::vector<haplotype_key>& keys,
                      int max_radius, int num_limit, neighbors_result& out, int device = 0);

// ---- wepp_filter::filter (initial_filter.cpp:455-506) ------------------------------------------------------------------
static constexpr int TOP_N = 10, MAX_PEAKS = 300, MAX_PEAK_PEAK_MUTATION = 2;      // src/WEPP/config.hpp:19-22
static constexpr int MAX_NEIGHBORS_WEPP = 50, FREYJA_PEAKS_LIMIT = 5000;           // config.hpp:20,23
struct peaks_params { int top_n = TOP_N, max_peaks = MAX_PEAKS, peak_radius = MAX_PEAK_PEAK_MUTATION; };

// cartesian_map and `while (!step(...))` (:465-469) in one device call (wepp_epp_peaks).  Haplotypes are arena indices.
struct peaks_result {
    cartesian_map_result map;                      // what the loop started from (epp_positions_cache is not filled)
    std::vector<haplotype_key> keys;               // what score_comparator reads, with the ORIGINAL scores
    std::vector<int> peaks, peak_step, peak_reads; // selection order; reads removed for the peak
    std::vector<long long> peak_degree;            // ... and the sum of their degrees
    std::vector<double> peak_score;                // full_score when chosen
    std::vector<int> removed_step, removed_peak;   // per read: the step and the place in `peaks`, -1 for a read that remains
    std::vector<char> mapped;                      // per haplotype
    int n_steps = 0, n_remaining = 0;
};
// The order among haplotypes whose full scores tie is score_comparator's: more leaves first (haplotype_leaf_counts
// over node_mappings), then the larger identifier.  Returns 0, or 1 after printing the error.
int wepp_filter_peaks(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                      const std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings, const peaks_params& params,
                      peaks_result& out, int device = 0);

// the whole of filter(): the loop, then the five expansion rounds (:473-504) -- per round k one wepp_epp_neighbors call
// (radius peak_radius + k, pivot->mutation_distance(node), nothing skipped), expand_peaks (neighbor_rank.hpp) on the
// original scores, and the round whose peaks + neighbours come closest to FREYJA_PEAKS_LIMIT is kept (the earlier one
// of two equally close)
struct filter_result {
    peaks_result loop;
    std::vector<int> neighbors;                    // ascending arena indices
    int round = -1;                                // the round kept (-1: none added anything to an empty set)
    std::vector<int> selection;                    // filter()'s return value: the peaks ascending, then the neighbours
};
int wepp_filter_filter(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                       const std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings, const peaks_params& params,
                       filter_result& out, int device = 0);
