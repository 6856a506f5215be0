// haplotype_report_main.cpp -- the host routines of wepp_amd/host/haplotype_report.cpp as a program of its own
// (tests/test_haplotype_report.py builds it plain and under AddressSanitizer + UBSan) for the tree of a .pb file:
//   haplotype_report_main tree.pb ref.fa
// prints, nodes in pre-order:
//   name <first token of the FASTA header>
//   geno <id> <pos>:<ref>:<mut> ...              get_mutations (through one genotype_lister, and by identifier)
//   words <id> <packed word> ...                 packed_genotypes
//   row <haplotype_row>                          (with its own newline)
//   dist <id a> <id b> <d>                       mutation_distance of every node against the node 7 places on, both ways
//   unc <uncertainty_row of the node, its parent and the root>
//   truth <truth_row>
//   keep <keep_positions> <words as hex>         keep_bits_of the positions of the last node's genotype
#include <cstdio>
#include <exception>
#include <fstream>

#include "../../wepp_amd/host/haplotype_report.hpp"

static std::string load_sequence(const char* path) {
    std::ifstream f(path);
    std::string line, seq;
    std::getline(f, line);
    while (std::getline(f, line)) for (char c : line) seq += (char)toupper(c);
    return seq;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: haplotype_report_main tree.pb ref.fa\n"); return 2; }
    try {
        MAT::Tree T = MAT::load_mutation_annotated_tree(argv[1]);
        T.uncondense_leaves();
        const std::string reference = load_sequence(argv[2]), ref_name = load_reference_name(argv[2]);
        printf("name %s\n", ref_name.c_str());
        std::vector<MAT::Node*> dfs = T.depth_first_expansion();
        genotype_lister lister;
        std::vector<std::vector<MAT::Mutation>> geno;
        packed_genotypes packed;
        for (MAT::Node* n : dfs) {
            geno.push_back(lister.get_mutations(n));
            std::vector<MAT::Mutation> again = get_mutations(T, n->identifier);
            if (again.size() != geno.back().size()) { fprintf(stderr, "the two get_mutations differ at %s\n", n->identifier.c_str()); return 1; }
            printf("geno %s", n->identifier.c_str());
            for (size_t i = 0; i < again.size(); i++) {
                const MAT::Mutation &m = geno.back()[i], &o = again[i];
                if (m.position != o.position || m.mut_nuc != o.mut_nuc || m.par_nuc != m.ref_nuc) { fprintf(stderr, "the two get_mutations differ at %s\n", n->identifier.c_str()); return 1; }
                printf(" %d:%d:%d", m.position, (int)m.ref_nuc, (int)m.mut_nuc);
            }
            printf("\n");
            packed.add(geno.back());
        }
        if (packed.size() != dfs.size()) return 1;
        for (size_t k = 0; k < dfs.size(); k++) {
            printf("words %s", dfs[k]->identifier.c_str());
            for (uint64_t i = packed.item_off[k]; i < packed.item_off[k + 1]; i++) printf(" %u", packed.item_word[i]);
            printf("\n");
            printf("row %s", haplotype_row(dfs[k]->identifier, ref_name, reference, geno[k]).c_str());
            const size_t o = (k + 7) % dfs.size();
            printf("dist %s %s %d\n", dfs[k]->identifier.c_str(), dfs[o]->identifier.c_str(), mutation_distance(geno[k], geno[o]));
            printf("dist %s %s %d\n", dfs[o]->identifier.c_str(), dfs[k]->identifier.c_str(), mutation_distance(geno[o], geno[k]));
            std::vector<MAT::Node*> src{dfs[k]};
            if (dfs[k]->parent) { src.push_back(dfs[k]->parent); src.push_back(T.root); }
            printf("unc %s", uncertainty_row((int)k, src).c_str());
            printf("truth %s", truth_row((int)(k % 120), dfs[k]->identifier, dfs[o]->identifier).c_str());
        }
        std::unordered_set<int> sites;
        for (const MAT::Mutation& m : geno.back()) sites.insert(m.position);
        uint32_t keep_positions = 0;
        std::vector<uint32_t> bits = keep_bits_of(sites, &keep_positions);
        printf("keep %u", keep_positions);
        for (uint32_t b : bits) printf(" %x", b);
        printf("\n");
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
