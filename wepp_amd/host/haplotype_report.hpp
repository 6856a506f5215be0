// haplotype_report.hpp -- host side of the last outputs of pipeline::run_from_last_initial that rest on the genotypes
// of full-tree nodes: dump_haplotype_uncertainty (src/WEPP/arena.cpp:494-528), dump_haplotypes (:906-931) and
// print_mutation_distance (:251-301).  The pairwise distances themselves are the device's (wepp_geno_diameters,
// wepp_geno_nearest; wepp_epp_cli.cpp makes the calls); here are the genotype of a node, the lists the C-ABI takes,
// and the rows as the reference prints them.  Host code only: tests/cxx/haplotype_report_main.cpp runs it under
// AddressSanitizer.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_set>
#include <vector>

#include "mat.hpp"

// get_mutations (util.cpp:271-296) of many nodes of one tree: the deepest mutation per position on the way from the
// node to the root, entries with mut_nuc == ref_nuc dropped (masked mutations, zeroed by the loader, with them),
// par_nuc = ref_nuc, sorted by position.  Linear in the path: a stamp per position says whether this walk has met
// it, where the reference searches its list for every mutation.
class genotype_lister {
  public:
    std::vector<MAT::Mutation> get_mutations(const MAT::Node* node);
  private:
    std::vector<uint32_t> stamp;       // per position: the walk that met it last
    uint32_t walk = 0;
};
// the reference's signature (node by identifier; unknown: empty, as rsearch returns no ancestors)
std::vector<MAT::Mutation> get_mutations(const MAT::Tree& T, const std::string& sample);
// mutation_distance (util.cpp:188-222) on lists sorted by position: the single-threaded merge
int mutation_distance(const std::vector<MAT::Mutation>& a, const std::vector<MAT::Mutation>& b);

// genotypes as the C-ABI takes them (wepp_genotypes): one wepp_pack_read_word per entry
struct packed_genotypes {
    std::vector<uint64_t> item_off{0};
    std::vector<uint32_t> item_word;
    void add(const std::vector<MAT::Mutation>& geno);
    uint32_t size() const { return (uint32_t)(item_off.size() - 1); }
};
// a set of sites as keep_bits over positions [0, keep_positions): keep_positions = the largest site + 1
std::vector<uint32_t> keep_bits_of(const std::unordered_set<int>& sites, uint32_t* keep_positions);

// dataset::reference_name (dataset.hpp:151-176): the first token of the FASTA header; throws MAT::mat_error
std::string load_reference_name(std::string const& fasta_filename);
// the MD:Z value of dump_haplotypes (arena.cpp:917-927)
std::string md_string(size_t genome_size, const std::vector<MAT::Mutation>& geno);
// one row of haplotypes.tsv (:912-929), with its newline
std::string haplotype_row(const std::string& id, const std::string& ref_name, const std::string& reference, const std::vector<MAT::Mutation>& geno);
// one row of haplotype_uncertainty.csv (:518-526), with its newline
std::string uncertainty_row(int max_dist, const std::vector<MAT::Node*>& sources);
// one row of print_mutation_distance (:297)
std::string truth_row(int min_dist, const std::string& true_id, const std::string& pred_id);
