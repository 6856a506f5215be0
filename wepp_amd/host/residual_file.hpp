// residual_file.hpp -- the reader of residual_mutations.txt (arena::resolve_unaccounted_mutations,
// src/WEPP/arena.cpp:708-731): one residual mutation per line, `<pos><letter>,<v1>[,<v2>...]`.  The key of a line, under
// which the reference files it (:760), is `<pos><letter>:<v1>:<v2>...`.  Plain C++ on top of the nucleotide codec of
// mat.hpp; see wepp_filter.hpp.
//
// Deliberately narrower than the reference's parser, which takes whatever std::stoi and substr make of a line:
//   - a line without a comma is an error (the reference would file the whole line as its own value);
//   - the part before the comma must be digits followed by ONE letter;
//   - the letter must round-trip through the codec (get_nuc(get_nuc_id(c)) == c): upper-case IUPAC codes except N
//     -- a residual N says nothing -- and except V, which the codec reads as N (MAT::get_nuc_id has no case 'V');
//   - the position must lie in 1 .. genome size, and the reference base there must be one of A, C, G, T;
//   - an exactly repeated line is an error (the reference would list the reads of the mutation twice under one key).
// Empty lines are skipped.
#pragma once
#include <cstdint>
#include <istream>
#include <string>
#include <unordered_set>
#include <vector>

#include "mat.hpp"

struct residual_mutation {
    int position = 0;
    char nuc = 'N';
    int8_t ref_nuc = 0, mut_nuc = 0;   // one-hot mask of the reference base; mask of the letter
    std::string key;                   // <pos><letter>:<v1>:<v2>...
};

inline std::vector<residual_mutation> parse_residual_mutations(std::istream& in, std::string const& filename,
                                                               std::string const& reference) {
    std::vector<residual_mutation> out;
    std::unordered_set<std::string> seen;
    std::string line;
    size_t lineno = 0;
    while (std::getline(in, line)) {
        lineno++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const std::string where = "ERROR: " + filename + ":" + std::to_string(lineno) + ": ";
        const size_t comma = line.find(',');
        if (comma == std::string::npos) throw MAT::mat_error(where + "no comma in '" + line + "'");
        const std::string mut = line.substr(0, comma);
        if (mut.size() < 2 || mut.size() > 10) throw MAT::mat_error(where + "'" + mut + "' is not <position><letter>");
        long pos = 0;
        for (size_t i = 0; i + 1 < mut.size(); i++) {
            if (mut[i] < '0' || mut[i] > '9') throw MAT::mat_error(where + "'" + mut + "' is not <position><letter>");
            pos = pos * 10 + (mut[i] - '0');
        }
        residual_mutation r;
        r.nuc = mut.back();
        r.mut_nuc = MAT::get_nuc_id(r.nuc);
        if (r.mut_nuc < 1 || r.mut_nuc > 14 || MAT::get_nuc(r.mut_nuc) != r.nuc)
            throw MAT::mat_error(where + "'" + std::string(1, r.nuc) + "' is not an allele the nucleotide codec maps both ways");
        if (pos < 1 || (size_t)pos > reference.size())
            throw MAT::mat_error(where + "position " + std::to_string(pos) + " is outside the reference (" +
                                 std::to_string(reference.size()) + " bases)");
        r.position = (int)pos;
        r.ref_nuc = MAT::get_nuc_id(reference[(size_t)pos - 1]);
        if (r.ref_nuc != 1 && r.ref_nuc != 2 && r.ref_nuc != 4 && r.ref_nuc != 8)
            throw MAT::mat_error(where + "the reference base at " + std::to_string(pos) + " is not one of A, C, G, T");
        r.key = mut;
        size_t at = comma + 1;                                  // the values, ',' -> ':' (:715-726)
        for (;;) {
            const size_t next = line.find(',', at);
            r.key += ":" + line.substr(at, next == std::string::npos ? std::string::npos : next - at);
            if (next == std::string::npos) break;
            at = next + 1;
        }
        if (!seen.insert(r.key).second) throw MAT::mat_error(where + "'" + line + "' is listed more than once");
        out.push_back(std::move(r));
    }
    return out;
}
