// clade_names.hpp -- the numbering of clade names wepp_mat_set_clades asks for (include/wepp_place.h): per annotation
// column the distinct names and "UNDEFINED", numbered 1, 2, .. by their rank under std::string::operator<, so that
// ascending id is the order std::sort leaves Missing_Sample::clade_assignments[c] in (usher_common.cpp:614).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mat.hpp"

struct CladeNumbering {
    std::vector<std::vector<std::string>> names;   // names[c][id - 1]
    std::vector<uint32_t> clade_id;                // [c * n_nodes + node], 0 = not annotated
    std::vector<uint32_t> undefined_id;            // [c]
    const std::string& name(size_t c, uint32_t id) const { return names[c][id - 1]; }
};

// nodes[i] = the node the C-ABI knows as id i
inline CladeNumbering number_clades(const std::vector<MAT::Node*>& nodes, size_t n_columns) {
    CladeNumbering out;
    const size_t n = nodes.size();
    out.names.resize(n_columns);
    out.clade_id.assign(n_columns * n, 0u);
    out.undefined_id.assign(n_columns, 0u);
    for (size_t c = 0; c < n_columns; c++) {
        std::vector<std::string>& names = out.names[c];
        names.emplace_back("UNDEFINED");
        for (const MAT::Node* nd : nodes)
            if (nd->clade_annotations.size() > c && !nd->clade_annotations[c].empty()) names.push_back(nd->clade_annotations[c]);
        std::sort(names.begin(), names.end());
        names.erase(std::unique(names.begin(), names.end()), names.end());
        auto id_of = [&](const std::string& s) { return (uint32_t)(std::lower_bound(names.begin(), names.end(), s) - names.begin()) + 1u; };
        out.undefined_id[c] = id_of("UNDEFINED");
        for (size_t i = 0; i < n; i++) {
            const MAT::Node* nd = nodes[i];
            if (nd->clade_annotations.size() > c && !nd->clade_annotations[c].empty()) out.clade_id[c * n + i] = id_of(nd->clade_annotations[c]);
        }
    }
    return out;
}
