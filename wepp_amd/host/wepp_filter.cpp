// wepp_filter.cpp -- see wepp_filter.hpp (citations: /root/reference/src/WEPP/).
#include "wepp_filter.hpp"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>

#include "../../include/wepp_place.h"
#include "pbwire.hpp"

using MAT::mat_error;
namespace pbwire = MAT::pbwire;

std::string load_reference(std::string const& fasta_filename) {
    std::ifstream fasta_f(fasta_filename);
    if (!fasta_f.is_open()) throw mat_error("Error: Unable to open file " + fasta_filename);
    std::string header, temp, ref_seq;
    std::getline(fasta_f, header);
    while (std::getline(fasta_f, temp)) {
        if (!temp.empty() && temp.back() == '\r') temp.pop_back();
        std::transform(temp.begin(), temp.end(), temp.begin(), [](unsigned char c) { return (char)std::toupper(c); });
        ref_seq += temp;
    }
    return ref_seq;
}

std::vector<int> load_masked_sites(std::string const& bed_filename) {
    std::vector<int> mask;
    std::ifstream in(bed_filename);
    if (!in.is_open()) return mask;                       // assume no masks
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string c1, c2;
        int c3;
        if (ls >> c1 >> c2 >> c3) mask.push_back(c3);
    }
    return mask;
}

std::vector<raw_read> load_reads_from_proto(std::string const& reference, std::string const& filename,
                                            std::unordered_map<std::string, std::vector<std::string>>& reverse_merge) {
    std::string raw = pbwire::slurp(filename, "read protobuf");
    pbwire::Wire top{(const uint8_t*)raw.data(), (const uint8_t*)raw.data() + raw.size()};
    std::vector<raw_read> reads;
    while (!top.eof()) {
        uint64_t key = top.varint();
        uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
        if (field == 1 && wt == 2) {                      // read_info
            pbwire::Wire w = top.sub();
            std::string name, content;
            int start_idx = 0, degree = 0;
            while (!w.eof()) {
                uint64_t k = w.varint();
                uint32_t f = (uint32_t)(k >> 3), t = (uint32_t)(k & 7);
                if (f == 1 && t == 2) name = w.str();
                else if (f == 3 && t == 0) start_idx = (int)(int32_t)w.varint();
                else if (f == 6 && t == 2) content = w.str();
                else if (f == 5 && t == 0) degree = (int)(int32_t)w.varint();
                else w.skip(t);
            }
            raw_read out;
            out.start = start_idx;
            out.end = start_idx + (int)content.size() - 1;
            out.degree = degree;
            out.read = name;
            if (start_idx < 1 || (size_t)out.end > reference.size())
                throw mat_error("ERROR: read " + name + " does not lie inside the reference");
            for (size_t i = 0; i < content.size(); ++i) {
                const char ref_c = reference[(size_t)start_idx + i - 1];
                if (content[i] != ref_c && content[i] != '_') {
                    MAT::Mutation m;
                    m.is_missing = content[i] == 'N';
                    m.ref_nuc = m.par_nuc = MAT::get_nuc_id(ref_c);
                    m.mut_nuc = MAT::get_nuc_id(content[i]);
                    m.position = out.start + (int)i;
                    out.mutations.push_back(std::move(m));
                }
            }
            reads.push_back(std::move(out));
        } else if (field == 2 && wt == 2) {               // column_info
            pbwire::Wire w = top.sub();
            std::string col;
            std::vector<std::string> inputs;
            while (!w.eof()) {
                uint64_t k = w.varint();
                uint32_t f = (uint32_t)(k >> 3), t = (uint32_t)(k & 7);
                if (f == 1 && t == 2) col = w.str();
                else if (f == 2 && t == 2) inputs.push_back(w.str());
                else w.skip(t);
            }
            for (auto& s : inputs) reverse_merge[col].push_back(s);
        } else {
            top.skip(wt);
        }
    }
    return reads;
}

static void put_read_info(std::string& out, sam_read_record const& r) {
    std::string m;
    pbwire::put_len(m, 1, r.name);
    pbwire::put_varint(m, (3u << 3) | 0);
    pbwire::put_varint(m, (uint64_t)(int64_t)r.start_idx);
    pbwire::put_varint(m, (5u << 3) | 0);
    pbwire::put_varint(m, (uint64_t)(int64_t)r.degree);
    pbwire::put_len(m, 6, r.content);
    pbwire::put_len(out, 1, m);
}

void dump_reads_proto(std::vector<sam_read_record> const& reads, std::string const& filename) {
    std::string out;
    for (auto const& r : reads) put_read_info(out, r);
    std::ofstream f(filename, std::ios::out | std::ios::binary);
    if (!f) throw mat_error("ERROR: Could not write the read protobuf: " + filename);
    f.write(out.data(), (std::streamsize)out.size());
}

void dump_reads_proto(std::vector<sam_read_record> const& reads, std::map<std::string, std::vector<std::string>> const& reverse_merge,
                      std::string const& filename) {
    const bool gz = filename.find(".gz") != std::string::npos;
    const std::string fail = "ERROR: Could not write the read protobuf: " + filename;
    gzFile zf = nullptr;
    std::ofstream f;
    if (gz) { zf = gzopen(filename.c_str(), "wb"); if (!zf) throw mat_error(fail); }
    else { f.open(filename, std::ios::out | std::ios::binary); if (!f) throw mat_error(fail); }
    std::string out;
    auto flush = [&](bool all) {                        // the message leaves in pieces: it is as large as the reads
        if (!all && out.size() < (1u << 22)) return;
        if (gz) { if (!out.empty() && gzwrite(zf, out.data(), (unsigned)out.size()) != (int)out.size()) { gzclose(zf); throw mat_error(fail); } }
        else f.write(out.data(), (std::streamsize)out.size());
        out.clear();
    };
    for (auto const& r : reads) { put_read_info(out, r); flush(false); }
    for (auto const& kv : reverse_merge) {
        std::string m;
        pbwire::put_len(m, 1, kv.first);
        for (auto const& name : kv.second) pbwire::put_len(m, 2, name);
        pbwire::put_len(out, 2, m);
        flush(false);
    }
    flush(true);
    if (gz) { if (gzclose(zf) != Z_OK) throw mat_error(fail); }
    else { f.close(); if (!f) throw mat_error(fail); }
}

void mask_reads(std::vector<raw_read>& reads, std::vector<int> const& masked_sites) {
    if (masked_sites.empty()) return;
    std::unordered_set<int> mask(masked_sites.begin(), masked_sites.end());
    for (auto& rd : reads)
        rd.mutations.erase(std::remove_if(rd.mutations.begin(), rd.mutations.end(),
                                          [&](const MAT::Mutation& m) { return mask.count(m.position) != 0; }),
                           rd.mutations.end());
}

std::unordered_set<int> site_read_map(std::vector<raw_read> const& reads, std::vector<int> const& masked_sites) {
    // A site is covered when some read spans it with a base other than N, and it is not masked:
    // (reads spanning j) - (reads with an N at j) > 0.  Both counts come from one pass over the reads
    // (a difference array over the genome for the spans), not from a walk over every base of every read.
    int last = 0;
    for (auto const& rd : reads) last = std::max(last, rd.end);
    std::vector<int32_t> span((size_t)last + 2, 0), n_at((size_t)last + 2, 0);
    for (auto const& rd : reads) {
        if (rd.end < rd.start) continue;
        const int lo = std::max(rd.start, 0);
        span[(size_t)lo] += 1;
        span[(size_t)rd.end + 1] -= 1;
        for (auto const& mut : rd.mutations)
            if (mut.mut_nuc == 0b1111 && mut.position >= lo && mut.position <= rd.end) n_at[(size_t)mut.position] += 1;
    }
    std::vector<char> masked((size_t)last + 2, 0);
    for (int site : masked_sites)
        if (site >= 0 && site <= last) masked[(size_t)site] = 1;
    std::unordered_set<int> covered;
    int32_t open_reads = 0;
    for (int j = 0; j <= last; j++) {
        open_reads += span[(size_t)j];
        if (open_reads - n_at[(size_t)j] > 0 && !masked[(size_t)j]) covered.insert(j);
    }
    return covered;
}

MAT::Tree create_condensed_tree(MAT::Node* ref_root, const std::unordered_set<int>& site_read_map,
                                std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings) {
    // Breadth-first order of the original tree; rep[k] = the condensed node that stands for original
    // node k: a new node when k keeps a mutation at a covered site (the root always), else the
    // representative of its parent.  Parents precede children in this order, and the children of a
    // condensed node are created in the order their originals appear in it -- which is what fixes the
    // pre-order (arena) index of every haplotype.
    MAT::Tree T;
    std::vector<MAT::Node*> order{ref_root};
    std::vector<size_t> parent_slot{0};
    for (size_t head = 0; head < order.size(); head++)
        for (MAT::Node* c : order[head]->children) { order.push_back(c); parent_slot.push_back(head); }
    std::vector<MAT::Node*> rep(order.size(), nullptr);
    for (size_t k = 0; k < order.size(); k++) {
        MAT::Node* orig = order[k];
        std::vector<MAT::Mutation> kept;
        std::copy_if(orig->mutations.begin(), orig->mutations.end(), std::back_inserter(kept),
                     [&](const MAT::Mutation& m) { return site_read_map.count(m.position) != 0; });
        if (k == 0 || !kept.empty()) {
            rep[k] = k == 0 ? T.create_node(orig->identifier, -1.0f)
                            : T.create_node(orig->identifier, rep[parent_slot[k]], -1.0f);
            rep[k]->mutations = std::move(kept);
            node_mappings[rep[k]] = {orig};
        } else {
            rep[k] = rep[parent_slot[k]];
            node_mappings[rep[k]].push_back(orig);
        }
    }
    return T;
}

namespace {

// the condensed tree as a device handle: node ids = BFS order (children of a node ascending = stored order), as in
// usher_place.cpp; bfs receives the nodes in that order
int make_handle(MAT::Tree& condensed, int device, std::vector<MAT::Node*>& bfs, wepp_mat_t** mat) {
    if (!condensed.root) {
        fprintf(stderr, "ERROR: empty tree!\n");
        return 1;
    }
    bfs = condensed.breadth_first_expansion();
    const size_t N = bfs.size();
    std::unordered_map<const MAT::Node*, int32_t> id;
    id.reserve(N * 2);
    for (size_t k = 0; k < N; k++) id[bfs[k]] = (int32_t)k;
    std::vector<int32_t> parent(N), mut_pos;
    std::vector<uint32_t> mut_off(N + 1, 0);
    std::vector<uint8_t> mut_ref, mut_par, mut_mut;
    for (size_t k = 0; k < N; k++) {
        parent[k] = bfs[k]->parent ? id[bfs[k]->parent] : -1;
        std::vector<MAT::Mutation> muts = bfs[k]->mutations;
        std::sort(muts.begin(), muts.end());               // arena.cpp:48
        for (auto& m : muts) {
            mut_pos.push_back(m.position);
            mut_ref.push_back((uint8_t)m.ref_nuc);
            mut_par.push_back((uint8_t)m.par_nuc);
            mut_mut.push_back((uint8_t)m.mut_nuc);
        }
        mut_off[k + 1] = (uint32_t)mut_pos.size();
    }
    wepp_tree_desc desc{(uint32_t)N, parent.data(), mut_off.data(), mut_pos.data(), mut_ref.data(), mut_par.data(),
                        mut_mut.data()};
    if (wepp_mat_create(&desc, device, mat) != WEPP_OK) {
        fprintf(stderr, "ERROR: %s\n", wepp_last_error());
        return 1;
    }
    return 0;
}

struct packed_reads {                // raw_reads as a wepp_epp_reads batch
    std::vector<uint32_t> off{0}, words;
    std::vector<int32_t> start, end, degree;
    explicit packed_reads(const std::vector<raw_read>& reads) : start(reads.size()), end(reads.size()), degree(reads.size()) {
        for (size_t r = 0; r < reads.size(); r++) {
            for (const MAT::Mutation& m : reads[r].mutations)
                words.push_back(wepp_pack_read_word((uint32_t)m.position, (uint32_t)m.ref_nuc, (uint32_t)m.mut_nuc,
                                                    m.mut_nuc == 0b1111 ? 1u : 0u));
            off.push_back((uint32_t)words.size());
            start[r] = reads[r].start; end[r] = reads[r].end; degree[r] = reads[r].degree;
        }
    }
    wepp_epp_reads view() const { return wepp_epp_reads{(uint32_t)start.size(), off.data(), words.data(), start.data(), end.data(), degree.data()}; }
};

}  // namespace

int cartesian_map(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                  cartesian_map_result& out, int device) {
    std::vector<MAT::Node*> bfs;
    wepp_mat_t* mat = nullptr;
    if (make_handle(condensed, device, bfs, &mat) != 0) return 1;
    const size_t N = bfs.size(), R = reads.size();
    packed_reads pr(reads);
    wepp_epp_reads in = pr.view();
    std::vector<int32_t> pars(R), counts(N * NUM_RANGE_BINS);
    std::vector<uint32_t> mult(R), epp, order(N);
    std::vector<uint64_t> epp_off(R + 1);
    out.score.assign(N, 0.0);
    out.dist_divergence.assign(N, 0.0);
    // The EPP lists hold what the reads' multiplicities add up to, at most MAX_CACHED_EPP_SIZE each: known only once
    // the map has run (the worst case, R * 2048 entries, is 8 GiB per million reads).  A typical guess first; when it is
    // short the map still delivers everything else and keeps the lists (WEPP_ELIMIT): they are fetched into a buffer
    // of the reported size -- the map itself runs ONCE.
    epp.resize(std::max<size_t>(R, 1) * 16);
    wepp_epp_out o{pars.data(), mult.data(), epp_off.data(), epp.data(), epp.size(), out.score.data(), counts.data(),
                   out.dist_divergence.data()};
    int rc = wepp_epp_map(mat, &in, (uint32_t)genome_size, MAX_CACHED_EPP_SIZE, &o);
    if (rc == WEPP_ELIMIT && epp_off[R] > epp.size()) {
        epp.assign((size_t)epp_off[R], 0);
        rc = wepp_epp_fetch_lists(mat, epp.data(), epp.size());
    }
    if (rc == WEPP_OK) rc = wepp_mat_dfs_order(mat, order.data());
    if (rc != WEPP_OK) {
        fprintf(stderr, "ERROR: %s\n", wepp_last_error());
        wepp_mat_destroy(mat);
        return 1;
    }
    wepp_mat_destroy(mat);
    out.haplotypes.resize(N);
    out.mapped_read_counts.resize(N);
    for (size_t k = 0; k < N; k++) {
        out.haplotypes[k] = bfs[order[k]];
        std::copy_n(&counts[k * NUM_RANGE_BINS], NUM_RANGE_BINS, out.mapped_read_counts[k].begin());
    }
    out.max_parismony.assign(pars.begin(), pars.end());
    out.parsimony_multiplicity.assign(mult.begin(), mult.end());
    out.epp_positions_cache.assign(R, {});
    for (size_t r = 0; r < R; r++)
        out.epp_positions_cache[r].assign(epp.begin() + (long)epp_off[r], epp.begin() + (long)epp_off[r + 1]);
    return 0;
}

namespace {

// sel[k] = arena index of selected[k]: the inverse of wepp_mat_dfs_order over the BFS ids
int arena_indices(wepp_mat_t* mat, const std::vector<MAT::Node*>& bfs, const std::vector<MAT::Node*>& selected,
                  std::vector<uint32_t>& sel) {
    const size_t N = bfs.size(), K = selected.size();
    std::vector<uint32_t> order(N);
    sel.assign(K, 0);
    if (wepp_mat_dfs_order(mat, order.data()) != WEPP_OK) {
        fprintf(stderr, "ERROR: %s\n", wepp_last_error());
        return 1;
    }
    std::unordered_map<const MAT::Node*, uint32_t> arena;
    arena.reserve(N * 2);
    for (size_t k = 0; k < N; k++) arena[bfs[order[k]]] = (uint32_t)k;
    for (size_t k = 0; k < K; k++) {
        auto it = arena.find(selected[k]);
        if (it == arena.end()) {
            fprintf(stderr, "ERROR: selected haplotype %zu is not a node of the condensed tree\n", k);
            return 1;
        }
        sel[k] = it->second;
    }
    return 0;
}

}  // namespace

int read2haplotype_mapping(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                           const std::vector<MAT::Node*>& selected, read2haplotype_result& out, int device) {
    std::vector<MAT::Node*> bfs;
    wepp_mat_t* mat = nullptr;
    if (make_handle(condensed, device, bfs, &mat) != 0) return 1;
    const size_t R = reads.size(), K = selected.size();
    std::vector<uint32_t> sel;
    if (arena_indices(mat, bfs, selected, sel) != 0) {
        wepp_mat_destroy(mat);
        return 1;
    }
    int rc = WEPP_OK;
    packed_reads pr(reads);
    wepp_epp_reads in = pr.view();
    std::vector<int32_t> min_dist(R);
    std::vector<uint32_t> n_epp(R), lists(std::max<size_t>(R, 1) * 4), sel_reads(K), covered(K);
    std::vector<uint64_t> off(R + 1, 0);
    std::vector<int64_t> degree(K);
    wepp_assign_out o{min_dist.data(), n_epp.data(), off.data(), lists.data(), lists.size(), sel_reads.data(), degree.data(),
                      covered.data(), nullptr};
    if (rc == WEPP_OK) rc = wepp_epp_assign(mat, &in, (uint32_t)genome_size, (uint32_t)K, sel.data(), &o);
    if (rc == WEPP_ELIMIT && off[R] > lists.size()) {
        // the guess was short: the sizes are known now, and a second call is cheap
        lists.assign((size_t)off[R], 0);
        o.asg_sel = lists.data();
        o.asg_capacity = lists.size();
        rc = wepp_epp_assign(mat, &in, (uint32_t)genome_size, (uint32_t)K, sel.data(), &o);
    }
    if (rc != WEPP_OK) fprintf(stderr, "ERROR: %s\n", wepp_last_error());
    wepp_mat_destroy(mat);
    if (rc != WEPP_OK) return 1;
    out.min_dist.assign(min_dist.begin(), min_dist.end());
    out.reads.assign(K, {});
    out.degree.assign(degree.begin(), degree.end());
    out.coverage.resize(K);
    for (size_t k = 0; k < K; k++) {
        out.reads[k].reserve(sel_reads[k]);
        out.coverage[k] = (double)covered[k] / (double)genome_size;      // arena.cpp:683-684
    }
    for (size_t r = 0; r < R; r++)                                      // ascending read index per haplotype
        for (uint64_t j = off[r]; j < off[r + 1]; j++) out.reads[lists[(size_t)j]].push_back((int)r);
    return 0;
}

std::vector<residual_mutation> load_residual_mutations(std::string const& filename, std::string const& reference) {
    std::ifstream in(filename);
    if (!in.is_open()) throw mat_error("Error: Unable to open file " + filename);
    return parse_residual_mutations(in, filename, reference);
}

int resolve_unaccounted_mutations(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                                  const std::vector<MAT::Node*>& selected, const std::vector<residual_mutation>& residual,
                                  resolve_result& out, int device) {
    std::vector<MAT::Node*> bfs;
    wepp_mat_t* mat = nullptr;
    if (make_handle(condensed, device, bfs, &mat) != 0) return 1;
    const size_t R = reads.size(), K = selected.size(), M = residual.size(), KW = (K + 31) / 32;
    std::vector<uint32_t> sel;
    if (arena_indices(mat, bfs, selected, sel) != 0) {
        wepp_mat_destroy(mat);
        return 1;
    }
    packed_reads pr(reads);
    wepp_epp_reads in = pr.view();
    std::vector<uint32_t> res(M), rel(std::max<size_t>(R, 1) * 4), n_cov(M), n_mask(M), best_mask(M * KW), touched(1);
    for (size_t m = 0; m < M; m++)
        res[m] = wepp_pack_read_word((uint32_t)residual[m].position, (uint32_t)residual[m].ref_nuc, (uint32_t)residual[m].mut_nuc, 0);
    std::vector<uint64_t> off(M + 1, 0);
    std::vector<int64_t> best_degree(M);
    wepp_resolve_out o{off.data(), rel.data(), rel.size(), n_cov.data(), n_mask.data(), best_degree.data(), best_mask.data(),
                       nullptr, nullptr, touched.data()};
    int rc = wepp_epp_resolve(mat, &in, (uint32_t)genome_size, (uint32_t)K, sel.data(), (uint32_t)M, res.data(), &o);
    if (rc == WEPP_ELIMIT && off[M] > rel.size()) {
        // the guess was short: the sizes are known now
        rel.assign((size_t)off[M], 0);
        o.rel_read = rel.data();
        o.rel_capacity = rel.size();
        rc = wepp_epp_resolve(mat, &in, (uint32_t)genome_size, (uint32_t)K, sel.data(), (uint32_t)M, res.data(), &o);
    }
    if (rc != WEPP_OK) fprintf(stderr, "ERROR: %s\n", wepp_last_error());
    wepp_mat_destroy(mat);
    if (rc != WEPP_OK) return 1;
    out.covered_reads.assign(M, {});
    out.n_masked.assign(n_mask.begin(), n_mask.end());
    out.best.assign(M, {});
    out.best_degree.assign(best_degree.begin(), best_degree.end());
    for (size_t m = 0; m < M; m++) {
        out.covered_reads[m].reserve(n_cov[m]);
        for (uint64_t j = off[m]; j < off[m + 1]; j++)
            if (!(rel[(size_t)j] >> 31)) out.covered_reads[m].push_back((int)rel[(size_t)j]);
        for (size_t k = 0; k < K; k++)
            if ((best_mask[m * KW + k / 32] >> (k & 31)) & 1u) out.best[m].push_back((int)k);
    }
    return 0;
}

std::vector<size_t> haplotype_leaf_counts(const std::vector<MAT::Node*>& haplotypes,
                                          const std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings) {
    std::vector<size_t> leaves(haplotypes.size(), 0);
    std::vector<MAT::Node*> remaining;
    for (size_t k = 0; k < haplotypes.size(); k++) {
        auto it = node_mappings.find(haplotypes[k]);
        if (it == node_mappings.end() || it->second.empty()) continue;
        remaining.assign(1, it->second.front());
        while (!remaining.empty()) {
            MAT::Node* curr = remaining.back();
            remaining.pop_back();
            if (curr->children.empty()) leaves[k]++;
            else remaining.insert(remaining.end(), curr->children.begin(), curr->children.end());
        }
    }
    return leaves;
}

std::vector<haplotype_key> haplotype_keys(const cartesian_map_result& map, const std::vector<size_t>& leaf_count) {
    std::vector<haplotype_key> keys(map.haplotypes.size());
    for (size_t k = 0; k < keys.size(); k++)
        keys[k] = haplotype_key{map.score[k] * std::sqrt(map.dist_divergence[k]), leaf_count[k], map.haplotypes[k]->identifier};
    return keys;
}

int closest_neighbors(MAT::Tree& condensed, const std::vector<MAT::Node*>& selected, const std::vector<haplotype_key>& keys,
                      int max_radius, int num_limit, neighbors_result& out, int device) {
    std::vector<MAT::Node*> bfs;
    wepp_mat_t* mat = nullptr;
    if (make_handle(condensed, device, bfs, &mat) != 0) return 1;
    const size_t K = selected.size();
    std::vector<uint32_t> piv;
    if (arena_indices(mat, bfs, selected, piv) != 0) {
        wepp_mat_destroy(mat);
        return 1;
    }
    if (keys.size() != bfs.size() || max_radius < 0) {
        fprintf(stderr, "ERROR: closest_neighbors: %zu keys for %zu haplotypes, radius %d\n", keys.size(), bfs.size(), max_radius);
        wepp_mat_destroy(mat);
        return 1;
    }
    std::vector<uint64_t> off(K + 1, 0);
    std::vector<uint32_t> node(std::max<size_t>(K, 1) * 64);
    std::vector<int32_t> dist(node.size());
    wepp_neighbors_out o{off.data(), node.data(), dist.data(), node.size(), nullptr, nullptr};
    int rc = wepp_epp_neighbors(mat, (uint32_t)K, piv.data(), (uint32_t)max_radius, WEPP_NBR_TO_PIVOT, nullptr, &o);
    if (rc == WEPP_ELIMIT && off[K] > node.size()) {
        // the guess was short: the sizes are known now
        node.assign((size_t)off[K], 0);
        dist.assign((size_t)off[K], 0);
        o.nbr_node = node.data(); o.nbr_dist = dist.data(); o.nbr_capacity = node.size();
        rc = wepp_epp_neighbors(mat, (uint32_t)K, piv.data(), (uint32_t)max_radius, WEPP_NBR_TO_PIVOT, nullptr, &o);
    }
    if (rc != WEPP_OK) fprintf(stderr, "ERROR: %s\n", wepp_last_error());
    wepp_mat_destroy(mat);
    if (rc != WEPP_OK) return 1;
    out.neighbors.assign(K, {});
    out.distance.assign(K, {});
    std::unordered_map<int, int> dist_of;
    for (size_t k = 0; k < K; k++) {
        std::vector<int> region(node.begin() + (long)off[k], node.begin() + (long)off[k + 1]);
        dist_of.clear();
        for (uint64_t j = off[k]; j < off[k + 1]; j++) dist_of[(int)node[(size_t)j]] = dist[(size_t)j];
        out.neighbors[k] = rank_neighbors(region, keys, num_limit);
        for (int h : out.neighbors[k]) out.distance[k].push_back(dist_of[h]);
    }
    out.next_selection = add_neighbors(out.neighbors, keys);
    return 0;
}

namespace {

// the loop on an open handle
int run_peaks(wepp_mat_t* mat, const std::vector<MAT::Node*>& bfs, const std::vector<raw_read>& reads, size_t genome_size,
              const std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings, const peaks_params& params,
              peaks_result& out) {
    const size_t N = bfs.size(), R = reads.size();
    if (params.top_n < 1 || params.max_peaks < 1 || params.peak_radius < 0) {
        fprintf(stderr, "ERROR: top_n and max_peaks must be at least 1 and peak_radius at least 0\n");
        return 1;
    }
    std::vector<uint32_t> order(N);
    if (wepp_mat_dfs_order(mat, order.data()) != WEPP_OK) {
        fprintf(stderr, "ERROR: %s\n", wepp_last_error());
        return 1;
    }
    cartesian_map_result& map = out.map;
    map.haplotypes.resize(N);
    for (size_t k = 0; k < N; k++) map.haplotypes[k] = bfs[order[k]];
    // score_comparator's last two criteria (arena.hpp:24-29) as a rank: more leaves first, then the larger identifier
    const std::vector<size_t> leaves = haplotype_leaf_counts(map.haplotypes, node_mappings);
    std::vector<uint32_t> by_rank(N), tie_rank(N);
    for (size_t k = 0; k < N; k++) by_rank[k] = (uint32_t)k;
    std::sort(by_rank.begin(), by_rank.end(), [&](uint32_t a, uint32_t b) {
        if (leaves[a] != leaves[b]) return leaves[a] > leaves[b];
        return map.haplotypes[a]->identifier > map.haplotypes[b]->identifier;
    });
    for (size_t k = 0; k < N; k++) tie_rank[by_rank[k]] = (uint32_t)k;

    packed_reads pr(reads);
    wepp_epp_reads in = pr.view();
    const uint32_t P = (uint32_t)params.max_peaks;
    std::vector<int32_t> pars(R), counts(N * NUM_RANGE_BINS), rstep(R);
    std::vector<uint32_t> mult(R), peaks(P), pstep(P), preads(P), rpeak(R);
    std::vector<int64_t> pdeg(P);
    std::vector<uint8_t> mapped(N);
    uint32_t n_peaks = 0, n_steps = 0, n_remaining = 0;
    map.score.assign(N, 0.0);
    map.dist_divergence.assign(N, 0.0);
    out.peak_score.assign(P, 0.0);
    wepp_epp_out mo{pars.data(), mult.data(), nullptr, nullptr, 0, map.score.data(), counts.data(), map.dist_divergence.data()};
    wepp_peaks_params pp{(uint32_t)params.top_n, P, (uint32_t)params.peak_radius, SCORE_EPSILON};
    wepp_peaks_out po{&n_peaks, &n_steps, &n_remaining, peaks.data(), pstep.data(), preads.data(), pdeg.data(), out.peak_score.data(),
                      rstep.data(), rpeak.data(), mapped.data(), nullptr};
    if (wepp_epp_peaks(mat, &in, (uint32_t)genome_size, &pp, tie_rank.data(), &mo, &po) != WEPP_OK) {
        fprintf(stderr, "ERROR: %s\n", wepp_last_error());
        return 1;
    }
    map.mapped_read_counts.resize(N);
    for (size_t k = 0; k < N; k++) std::copy_n(&counts[k * NUM_RANGE_BINS], NUM_RANGE_BINS, map.mapped_read_counts[k].begin());
    map.max_parismony.assign(pars.begin(), pars.end());
    map.parsimony_multiplicity.assign(mult.begin(), mult.end());
    map.epp_positions_cache.assign(R, {});
    out.keys = haplotype_keys(map, leaves);
    out.peaks.assign(peaks.begin(), peaks.begin() + n_peaks);
    out.peak_step.assign(pstep.begin(), pstep.begin() + n_peaks);
    out.peak_reads.assign(preads.begin(), preads.begin() + n_peaks);
    out.peak_degree.assign(pdeg.begin(), pdeg.begin() + n_peaks);
    out.peak_score.resize(n_peaks);
    out.removed_step.assign(rstep.begin(), rstep.end());
    out.removed_peak.resize(R);
    for (size_t r = 0; r < R; r++) out.removed_peak[r] = rpeak[r] == 0xFFFFFFFFu ? -1 : (int)rpeak[r];
    out.mapped.assign(mapped.begin(), mapped.end());
    out.n_steps = (int)n_steps;
    out.n_remaining = (int)n_remaining;
    return 0;
}

}  // namespace

int wepp_filter_peaks(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                      const std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings, const peaks_params& params,
                      peaks_result& out, int device) {
    std::vector<MAT::Node*> bfs;
    wepp_mat_t* mat = nullptr;
    if (make_handle(condensed, device, bfs, &mat) != 0) return 1;
    const int rc = run_peaks(mat, bfs, reads, genome_size, node_mappings, params, out);
    wepp_mat_destroy(mat);
    return rc;
}

int wepp_filter_filter(MAT::Tree& condensed, const std::vector<raw_read>& reads, size_t genome_size,
                       const std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings, const peaks_params& params,
                       filter_result& out, int device) {
    std::vector<MAT::Node*> bfs;
    wepp_mat_t* mat = nullptr;
    if (make_handle(condensed, device, bfs, &mat) != 0) return 1;
    if (run_peaks(mat, bfs, reads, genome_size, node_mappings, params, out.loop) != 0) {
        wepp_mat_destroy(mat);
        return 1;
    }
    const std::vector<int>& peaks = out.loop.peaks;
    const size_t K = peaks.size();
    out.neighbors.clear();
    out.round = -1;
    std::vector<uint32_t> piv(peaks.begin(), peaks.end());
    std::vector<uint64_t> off(K + 1, 0);
    std::vector<uint32_t> node(std::max<size_t>(K, 1) * 64);
    std::vector<int32_t> dist(node.size());
    for (int k = 0; k < 5 && K; k++) {                                         // :474
        const uint32_t radius = (uint32_t)(params.peak_radius + k);
        wepp_neighbors_out o{off.data(), node.data(), dist.data(), node.size(), nullptr, nullptr};
        int rc = wepp_epp_neighbors(mat, (uint32_t)K, piv.data(), radius, WEPP_NBR_FROM_PIVOT, nullptr, &o);
        if (rc == WEPP_ELIMIT && off[K] > node.size()) {
            node.assign((size_t)off[K], 0);
            dist.assign((size_t)off[K], 0);
            o.nbr_node = node.data(); o.nbr_dist = dist.data(); o.nbr_capacity = node.size();
            rc = wepp_epp_neighbors(mat, (uint32_t)K, piv.data(), radius, WEPP_NBR_FROM_PIVOT, nullptr, &o);
        }
        if (rc != WEPP_OK) {
            fprintf(stderr, "ERROR: %s\n", wepp_last_error());
            wepp_mat_destroy(mat);
            return 1;
        }
        std::vector<std::vector<int>> regions(K);
        for (size_t j = 0; j < K; j++) regions[j].assign(node.begin() + (long)off[j], node.begin() + (long)off[j + 1]);
        std::vector<int> curr = expand_peaks(peaks, regions, out.loop.keys, MAX_NEIGHBORS_WEPP);
        if (std::abs(FREYJA_PEAKS_LIMIT - (int)(curr.size() + K)) < std::abs(FREYJA_PEAKS_LIMIT - (int)(out.neighbors.size() + K))) {   // :499
            out.neighbors.swap(curr);
            out.round = k;
        }
    }
    wepp_mat_destroy(mat);
    out.selection.assign(peaks.begin(), peaks.end());
    std::sort(out.selection.begin(), out.selection.end());                     // (std::set<haplotype*>: arena order)
    out.selection.insert(out.selection.end(), out.neighbors.begin(), out.neighbors.end());
    return 0;
}
