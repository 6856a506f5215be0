// clades_host_main.cpp -- the host-only code of the clade assignment as a program of its own (tests/test_host_clades.py
// builds it plain and under AddressSanitizer + UBSan): the loader's clade_annotations, Tree::get_clade_assignment,
// the numbering of the names (wepp_amd/host/clade_names.hpp) and the two ancestor tables of wepp_mat_set_clades
// (wepp_amd/csrc/clades_host.hpp) for the tree of a .pb file.
//   clades_host_main tree.pb
// prints, with the node ids the C-ABI would see (BFS index):
//   columns <C>
//   name <c> <id>\t<name>                        the numbering
//   assign <c> <node>\t<self>\t<ancestors>       get_clade_assignment(node, c, true / false)
//   table <c> <node> <id self> <id ancestors>    the tables, by node (through the pre-order they are built in)
#include <cstdio>
#include <exception>
#include <vector>

#include "../../wepp_amd/csrc/clades_host.hpp"
#include "../../wepp_amd/host/clade_names.hpp"
#include "../../wepp_amd/host/mat.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: clades_host_main tree.pb\n"); return 2; }
    try {
        MAT::Tree T = MAT::load_mutation_annotated_tree(argv[1]);
        T.uncondense_leaves();
        const size_t C = T.get_num_annotations();
        std::vector<MAT::Node*> bfs = T.breadth_first_expansion(), dfs = T.depth_first_expansion();
        const uint32_t N = (uint32_t)bfs.size();
        printf("columns %zu\n", C);
        CladeNumbering num = number_clades(bfs, C);
        for (size_t c = 0; c < C; c++)
            for (size_t i = 0; i < num.names[c].size(); i++) printf("name %zu %zu\t%s\n", c, i + 1, num.names[c][i].c_str());
        for (size_t c = 0; c < C; c++)
            for (uint32_t i = 0; i < N; i++)
                printf("assign %zu %u\t%s\t%s\n", c, i, T.get_clade_assignment(bfs[i], (int)c, true).c_str(),
                       T.get_clade_assignment(bfs[i], (int)c, false).c_str());
        // ids: dfs_idx is set by depth_first_expansion; the BFS index of a node through a table over dfs_idx
        std::vector<uint32_t> dfs2id(N), parent_dfs(N, 0);
        for (uint32_t i = 0; i < N; i++) dfs2id[bfs[i]->dfs_idx] = i;
        for (uint32_t d = 0; d < N; d++) parent_dfs[d] = dfs[d]->parent ? (uint32_t)dfs[d]->parent->dfs_idx : 0u;
        std::vector<uint32_t> tab;
        wepp::clade_build_tables(N, (uint32_t)C, parent_dfs.data(), dfs2id.data(), num.clade_id.data(), num.undefined_id.data(), tab);
        for (size_t c = 0; c < C; c++)
            for (uint32_t d = 0; d < N; d++)
                printf("table %zu %u %u %u\n", c, dfs2id[d], tab[(c * 2 + 1) * N + d], tab[(c * 2) * N + d]);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
