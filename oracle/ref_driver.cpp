/*
 * oracle/ref_driver.cpp -- serial driver around the REFERENCE's own placement scorer.
 *
 * TEST INFRASTRUCTURE ONLY.  tests/ref_bridge.py compiles this file together with the reference's
 * src/usher_mapper.cpp (unchanged) and the needed stretches of its src/mutation_annotated_tree.cpp into
 * oracle/_ref/ref_driver; the stand-ins of oracle/ref_shim/ replace TBB, Boost and protobuf.  Everything that
 * scores, breaks ties, walks the tree or assigns a clade below is the reference's code: mapper2_body,
 * Tree::create_node, Node::add_mutation, Tree::breadth_first_expansion, Tree::get_num_leaves,
 * Tree::get_clade_assignment.  What is restated here, with its cite (relative to the reference's src/):
 *   the loader's rule for a node's list      mutation_annotated_tree.cpp:580-594
 *   the per-sample loop and its first values usher_common.cpp:339-446 (serial where the reference has
 *                                            tbb::parallel_for, once ascending and once descending)
 *   the clade loop                           usher_common.cpp:597-615 (its guards max_uncertainty / max_parsimony
 *                                            default to 1e6 and are not applied)
 *
 * Input (whitespace-separated tokens, from the file named on the command line or stdin):
 *   WEPPREF 1 <full|digest> <n_trees>
 *   per tree:   <n_nodes> <n_columns> <n_samples>
 *     per node (id order, parent < id, node 0 the root):  <parent> <n_muts> then n_muts x <pos> <ref> <par> <mut>
 *     per column, per node:                                =<annotation>   ("=" alone: none)
 *     per sample:                                          <k> then k x <pos> <ref> <mut> <is_missing>
 * Mutation nucleotides are passed on exactly as given, those of masked mutations (pos < 0) included.
 *
 * Output: one JSON line per tree: {"bfs": [...], "results": [per sample {"asc": RUNS, "desc": RUNS}]} with
 * RUNS = {"p": {...}, "place": {...}}: the -p mode and the two-pass placement mode in that node order.
 * "lists" is a digest over the imputed and excess lists of every node (oracle_lists_digest() in
 * oracle/mapper2_oracle.c computes the same number), "excess_listed" one over the excess lists alone; `full` also
 * writes the lists themselves (ascending run) and the descending run's per-node scores, of which `digest` keeps a
 * digest.
 */
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "usher_graph.hpp"

namespace {

struct Digest {                                  /* FNV-1a over 32-bit words */
    uint64_t h = 1469598103934665603ull;
    void add(int32_t w) { h = (h ^ (uint64_t)(uint32_t)w) * 1099511628211ull; }
    void add(const std::vector<MAT::Mutation> &v) {
        add((int32_t)v.size());
        for (auto &m : v) { add(m.position); add(m.ref_nuc); add(m.par_nuc); add(m.mut_nuc); }
    }
};

struct Run {
    int score = 0;
    size_t num_best = 0, best_j = 0;
    bool has_unique = false;
    MAT::Node *best_node = nullptr;
    std::vector<size_t> best_j_vec;              /* in the order the reference pushed them */
    std::vector<bool> node_has_unique;
    std::vector<int> node_scores;                /* -p mode only */
    std::vector<std::vector<MAT::Mutation>> excess, imputed;
};

std::vector<size_t> node_order(size_t n, bool descending) {
    std::vector<size_t> o(n);
    for (size_t i = 0; i < n; i++) o[i] = descending ? n - 1 - i : i;
    return o;
}

/* usher_common.cpp:339-446 for one sample; `order` replaces the blocked ranges of tbb::parallel_for */
Run run_sample(MAT::Tree *T, std::vector<MAT::Node *> &bfs, std::vector<MAT::Mutation> &S, bool print_parsimony_scores,
               bool descending) {
    Run r;
    size_t total_nodes = bfs.size();                                            /* :340 */
    r.excess.resize(total_nodes);                                               /* :351 */
    r.imputed.resize(total_nodes);                                              /* :356 */
    if (print_parsimony_scores) r.node_scores.resize(total_nodes);              /* :360-362 */
    size_t best_node_num_leaves = 0;                                            /* :364 */
    int best_set_difference = S.size() + T->root->mutations.size() + 1;         /* :371 */
    size_t best_j = 0;                                                          /* :373 */
    bool best_node_has_unique = false;                                          /* :374 */
    r.node_has_unique.assign(total_nodes, false);                               /* :376 */
    r.best_j_vec.emplace_back(0);                                               /* :377-378 */
    size_t num_best = 1;                                                        /* :380 */
    MAT::Node *best_node = T->root;                                             /* :381 */

    auto fill = [&](mapper2_input &inp, size_t k) {                             /* :389-407, :427-442 */
        inp.T = T;
        inp.node = bfs[k];
        inp.missing_sample_mutations = &S;
        inp.excess_mutations = &r.excess[k];
        inp.imputed_mutations = &r.imputed[k];
        inp.best_node_num_leaves = &best_node_num_leaves;
        inp.best_set_difference = &best_set_difference;
        inp.best_node = &best_node;
        inp.best_j = &best_j;
        inp.num_best = &num_best;
        inp.j = k;
        inp.has_unique = &best_node_has_unique;
        if (print_parsimony_scores) inp.set_difference = &r.node_scores[k];
        inp.best_j_vec = &r.best_j_vec;
        inp.node_has_unique = &r.node_has_unique;
    };
    for (size_t k : node_order(total_nodes, descending)) {                      /* :386-411 */
        mapper2_input inp;
        fill(inp, k);
        mapper2_body(inp, print_parsimony_scores, print_parsimony_scores);      /* :409 */
    }
    if (!print_parsimony_scores) {                                              /* :413-446 */
        /* second pass: the bound one above the best found, the counters emptied, the first pass's nodes again */
        const std::vector<size_t> again(r.best_j_vec);
        best_set_difference += 1;
        num_best = 0;
        r.best_j_vec.clear();
        for (size_t k : again) {
            mapper2_input inp;
            fill(inp, k);
            mapper2_body(inp, false);                                           /* :444: compute_vecs by default */
        }
    }
    r.score = best_set_difference;
    r.num_best = num_best;
    r.best_j = best_j;
    r.has_unique = best_node_has_unique;
    r.best_node = best_node;
    return r;
}

void put_list(std::string &o, const std::vector<MAT::Mutation> &v, bool four) {
    o += "[";
    for (size_t i = 0; i < v.size(); i++) {
        if (i) o += ",";
        o += "[" + std::to_string(v[i].position) + ",";
        if (four) o += std::to_string((int)v[i].ref_nuc) + "," + std::to_string((int)v[i].par_nuc) + ",";
        o += std::to_string((int)v[i].mut_nuc) + "]";
    }
    o += "]";
}

void put_string(std::string &o, const std::string &s) {
    o += "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    o += "\"";
}

/* the scalars, the sorted best_j_vec and node_has_unique of its nodes */
void put_common(std::string &o, const Run &r) {
    std::vector<size_t> v(r.best_j_vec);
    std::sort(v.begin(), v.end());
    o += "\"score\":" + std::to_string(r.score) + ",\"num_best\":" + std::to_string(r.num_best) +
         ",\"best_j\":" + std::to_string(r.best_j) + ",\"has_unique\":" + std::to_string((int)r.has_unique) + ",\"best_j_vec\":[";
    for (size_t i = 0; i < v.size(); i++) o += (i ? "," : "") + std::to_string(v[i]);
    o += "],\"node_has_unique\":[";
    for (size_t i = 0; i < v.size(); i++) o += (i ? "," : "") + std::to_string((int)r.node_has_unique[v[i]]);
    o += "]";
}

void fail(const char *what) {
    fprintf(stderr, "ref_driver: %s\n", what);
    exit(2);
}

}  // namespace

int main(int argc, char **argv) {
    std::ifstream file;
    if (argc > 1) {
        file.open(argv[1]);
        if (!file) fail("cannot open the input file");
    }
    std::istream &in = argc > 1 ? (std::istream &)file : std::cin;
    std::string magic, mode;
    int version = 0;
    long n_trees = 0;
    in >> magic >> version >> mode >> n_trees;
    if (!in || magic != "WEPPREF" || version != 1 || (mode != "full" && mode != "digest")) fail("bad header");
    const bool full = mode == "full";

    for (long t = 0; t < n_trees; t++) {
        long n_nodes, n_cols, n_samples;
        in >> n_nodes >> n_cols >> n_samples;
        if (!in || n_nodes < 1 || n_cols < 0 || n_samples < 0) fail("bad tree header");
        MAT::Tree T;
        std::vector<MAT::Node *> by_id((size_t)n_nodes);
        for (long i = 0; i < n_nodes; i++) {
            long parent, nm;
            in >> parent >> nm;
            if (!in || nm < 0 || (i == 0 ? parent != -1 : (parent < 0 || parent >= i))) fail("bad node line");
            /* ids in ascending order: children are pushed in the description's order (create_node, :865-878) */
            by_id[i] = i == 0 ? T.create_node(std::to_string(i), -1.0f, (size_t)n_cols)
                              : T.create_node(std::to_string(i), by_id[parent], -1.0f);
            MAT::Node *node = by_id[i];
            for (long k = 0; k < nm; k++) {
                long pos, ref, par, mut;
                in >> pos >> ref >> par >> mut;
                if (!in) fail("bad mutation");
                MAT::Mutation m;
                m.position = (int)pos;
                m.ref_nuc = (int8_t)ref;
                m.par_nuc = (int8_t)par;
                m.mut_nuc = (int8_t)mut;
                m.is_missing = false;
                /* mutation_annotated_tree.cpp:571-589: a mutation that changes nothing is dropped, a masked one is
                 * always added (its nucleotides are NOT zeroed here: they arrive as the description holds them) */
                if (m.is_masked() || m.mut_nuc != m.par_nuc) node->add_mutation(m);
            }
            if (!std::is_sorted(node->mutations.begin(), node->mutations.end()))             /* :591-594 */
                std::sort(node->mutations.begin(), node->mutations.end());
        }
        for (long c = 0; c < n_cols; c++)
            for (long i = 0; i < n_nodes; i++) {
                std::string tok;
                in >> tok;
                if (!in || tok.empty() || tok[0] != '=') fail("bad annotation");
                by_id[i]->clade_annotations[(size_t)c] = tok.substr(1);
            }

        auto bfs = T.breadth_first_expansion();                                              /* usher_common.cpp:339 */
        std::string o = "{\"bfs\":[";
        for (size_t k = 0; k < bfs.size(); k++) o += (k ? "," : "") + bfs[k]->identifier;
        o += "],\"results\":[";
        for (long s = 0; s < n_samples; s++) {
            long k;
            in >> k;
            if (!in || k < 0) fail("bad sample");
            std::vector<MAT::Mutation> S;
            for (long e = 0; e < k; e++) {
                long pos, ref, mut, missing;
                in >> pos >> ref >> mut >> missing;
                if (!in) fail("bad sample entry");
                MAT::Mutation m;
                m.position = (int)pos;
                m.ref_nuc = (int8_t)ref;
                m.par_nuc = (int8_t)ref;
                m.mut_nuc = (int8_t)mut;
                m.is_missing = missing != 0;
                S.emplace_back(m);
            }
            o += s ? ",{" : "{";
            for (int d = 0; d < 2; d++) {
                o += d ? ",\"desc\":{" : "\"asc\":{";
                Run p = run_sample(&T, bfs, S, true, d == 1);
                Digest dg;
                for (size_t j = 0; j < bfs.size(); j++) { dg.add(p.excess[j]); dg.add(p.imputed[j]); }
                o += "\"p\":{";
                put_common(o, p);
                o += ",\"lists\":\"" + std::to_string(dg.h) + "\"";
                /* the excess lists once more without their entries of position < 0 (a masked root mutation that
                 * carries nucleotides, which wepp_excess_mutations documents it does not list), and how many those were */
                Digest dx;
                size_t n_masked = 0;
                for (size_t j = 0; j < bfs.size(); j++) {
                    std::vector<MAT::Mutation> kept;
                    for (auto &m : p.excess[j]) {
                        if (m.is_masked()) n_masked++;
                        else kept.push_back(m);
                    }
                    dx.add(kept);
                }
                o += ",\"excess_listed\":\"" + std::to_string(dx.h) + "\",\"excess_masked\":" + std::to_string(n_masked);
                if (full || d == 0) {
                    o += ",\"node_scores\":[";
                    for (size_t j = 0; j < bfs.size(); j++) o += (j ? "," : "") + std::to_string(p.node_scores[j]);
                    o += "]";
                } else {
                    Digest ds;
                    for (int v : p.node_scores) ds.add(v);
                    o += ",\"node_scores_digest\":\"" + std::to_string(ds.h) + "\"";
                }
                if (full && d == 0) {
                    o += ",\"excess\":[";
                    for (size_t j = 0; j < bfs.size(); j++) { if (j) o += ","; put_list(o, p.excess[j], true); }
                    o += "],\"imputed\":[";
                    for (size_t j = 0; j < bfs.size(); j++) { if (j) o += ","; put_list(o, p.imputed[j], true); }
                    o += "]";
                }
                Run q = run_sample(&T, bfs, S, false, d == 1);
                o += "},\"place\":{";
                put_common(o, q);
                o += ",\"imputed_best\":";
                put_list(o, q.imputed[q.best_j], false);
                o += ",\"clades\":[";
                for (size_t c = 0; c < T.get_num_annotations(); c++) {                       /* usher_common.cpp:603-615 */
                    std::vector<std::string> names;
                    std::string best;
                    for (size_t j : q.best_j_vec) {              /* in the order pass 2 pushed them */
                        MAT::Node *cand = bfs[j];
                        const bool with_self = !cand->is_leaf() && !q.node_has_unique[j];            /* :607 */
                        names.push_back(T.get_clade_assignment(cand, (int)c, with_self));            /* :608-609 */
                        if (cand == q.best_node) best = names.back();                               /* :610-612 */
                    }
                    std::sort(names.begin(), names.end());
                    o += c ? ",[" : "[";
                    put_string(o, best);
                    o += ",[";
                    for (size_t kk = 0; kk < names.size(); kk++) { if (kk) o += ","; put_string(o, names[kk]); }
                    o += "]]";
                }
                o += "]}}";
            }
            o += "}";
        }
        o += "]}\n";
        fputs(o.c_str(), stdout);
        for (auto n : bfs) delete n;
        T.root = NULL;
    }
    return 0;
}
