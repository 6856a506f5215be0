// haplotype_report.cpp -- see haplotype_report.hpp
#include "haplotype_report.hpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>

#include "../../include/wepp_place.h"

std::vector<MAT::Mutation> genotype_lister::get_mutations(const MAT::Node* node) {
    std::vector<MAT::Mutation> out;
    if (++walk == 0) { std::fill(stamp.begin(), stamp.end(), 0u); walk = 1; }
    for (const MAT::Node* anc = node; anc; anc = anc->parent)
        for (const MAT::Mutation& mut : anc->mutations) {
            if (mut.position < 0) continue;                 // masked: ref_nuc == mut_nuc == 0, and one position for all of them
            if ((size_t)mut.position >= stamp.size()) stamp.resize((size_t)mut.position + 1, 0u);
            if (stamp[(size_t)mut.position] == walk) continue;   // a deeper node has spoken
            stamp[(size_t)mut.position] = walk;
            if (mut.ref_nuc == mut.mut_nuc) continue;       // back to the reference: no entry (the stamp still hides the ancestors')
            out.push_back(mut);
            out.back().par_nuc = mut.ref_nuc;
        }
    std::sort(out.begin(), out.end());
    return out;
}

std::vector<MAT::Mutation> get_mutations(const MAT::Tree& T, const std::string& sample) {
    genotype_lister lister;
    const MAT::Node* n = T.get_node(sample);
    return n ? lister.get_mutations(n) : std::vector<MAT::Mutation>();
}

int mutation_distance(const std::vector<MAT::Mutation>& a, const std::vector<MAT::Mutation>& b) {
    size_t i = 0, j = 0;
    int distance = 0;
    while (i < a.size() && j < b.size()) {
        if (a[i].position == b[j].position) {
            if (a[i].mut_nuc != b[j].mut_nuc) distance++;
            i++; j++;
        } else if (a[i].position < b[j].position) { distance++; i++; }
        else { distance++; j++; }
    }
    return distance + (int)(a.size() - i) + (int)(b.size() - j);
}

void packed_genotypes::add(const std::vector<MAT::Mutation>& geno) {
    for (const MAT::Mutation& m : geno)
        item_word.push_back(wepp_pack_read_word((uint32_t)m.position, (uint32_t)m.ref_nuc & 15u, (uint32_t)m.mut_nuc & 15u, 0));
    item_off.push_back(item_word.size());
}

std::vector<uint32_t> keep_bits_of(const std::unordered_set<int>& sites, uint32_t* keep_positions) {
    int top = -1;
    for (int s : sites) top = std::max(top, s);
    *keep_positions = (uint32_t)(top + 1);
    std::vector<uint32_t> bits(((size_t)*keep_positions + 31) / 32, 0u);
    for (int s : sites)
        if (s >= 0) bits[(size_t)s / 32] |= 1u << (s % 32);
    return bits;
}

std::string load_reference_name(std::string const& fasta_filename) {
    std::ifstream fasta_f(fasta_filename);
    if (!fasta_f.is_open()) throw MAT::mat_error("Error: Unable to open file " + fasta_filename);
    std::string line, name;
    std::getline(fasta_f, line);
    if (line.empty() || line[0] != '>') throw MAT::mat_error("Error: Fasta format NOT correct " + fasta_filename);
    std::istringstream iss(line.substr(1));
    iss >> name;
    return name;
}

std::string md_string(size_t genome_size, const std::vector<MAT::Mutation>& geno) {
    std::string md = "MD:Z:";
    int start_idx = 1;
    for (const MAT::Mutation& mut : geno) {
        md += std::to_string(mut.position - start_idx) + MAT::get_nuc(mut.ref_nuc);
        start_idx = mut.position + 1;
    }
    if (genome_size - (size_t)start_idx + 1) md += std::to_string(genome_size - (size_t)start_idx + 1);
    return md;
}

std::string haplotype_row(const std::string& id, const std::string& ref_name, const std::string& reference, const std::vector<MAT::Mutation>& geno) {
    std::string seq = reference;
    for (const MAT::Mutation& mut : geno) {
        if (mut.position < 1 || (size_t)mut.position > seq.size())
            throw MAT::mat_error("Error: haplotype " + id + " holds a mutation at " + std::to_string(mut.position) + ", outside the reference");
        seq[(size_t)mut.position - 1] = MAT::get_nuc(mut.mut_nuc);
    }
    return id + "\t0\t" + ref_name + "\t1\t60\t" + std::to_string(reference.size()) + "M\t*\t0\t0\t" + seq + "\t" + std::string(seq.size(), '?') + "\t" +
           md_string(reference.size(), geno) + "\tRG:Z:group\n";
}

std::string uncertainty_row(int max_dist, const std::vector<MAT::Node*>& sources) {
    std::string row;
    for (size_t i = 0; i < sources.size(); i++)
        row += i ? "," + sources[i]->identifier : std::to_string(max_dist) + "," + sources[i]->identifier;
    return row + "\n";
}

std::string truth_row(int min_dist, const std::string& true_id, const std::string& pred_id) {
    char head[32];
    snprintf(head, sizeof head, "* dist: %02d true_node: ", min_dist);
    return head + true_id + " pred_node: " + pred_id + " \n";
}
