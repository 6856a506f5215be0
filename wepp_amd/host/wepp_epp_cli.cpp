// wepp_epp_cli.cpp -- `wepp-epp`: the data path of `wepp detectPeaks` up to and including
// wepp_filter::cartesian_map, on files: MAT .pb[.gz] + reads .pb (sam.proto, as written by
// `wepp sam2PB`) + reference FASTA [+ mask.bed] -> haplotype scores and per-read placements.
//   wepp-epp -i tree.pb -r reads.pb -f ref.fa [-m mask.bed] -d outdir [--device N] [--dump] [--assign FILE [--resolve RESIDUAL]]
//            [--neighbors FILE [--radius R] [--max-neighbors L]] [--peaks [--top-n T] [--max-peaks P] [--peak-radius Q]]
//            [--clade-idx N] [--uncertainty] [--haplotypes] [--truth TRUE]   (the last three with --assign only)
// --dump prints what the loaders and the condensing step produced and exits (no GPU needed).
// Output: <outdir>/haplotype_scores.tsv (arena order: id, score, dist_divergence, sources),
//         <outdir>/read_placements.tsv  (read, start, end, degree, parsimony, epps).
// --assign FILE: FILE names the selected haplotypes, one identifier of a condensed node per line (anything after a
// tab or comma is ignored; an unknown or repeated identifier is an error).  A line that is no identifier but a number
// below the number of haplotypes is an arena index (the pre-order of the condensed tree): peaks.txt of --peaks.  After the map the reads are assigned to
// their nearest selected haplotypes (arena::dump_read2haplotype_mapping, arena.cpp:590-696, without the SAM files):
//         <outdir>/haplotype_reads.csv     one row per selected haplotype that has a read, in the order of FILE:
//                                          id,name,name,... -- the names reverse_merge (the reads file's column table) lists
//                                          for its reads, reads in input order.  The reference's row and
//                                          name order follow its hash map and thread schedule; this order is ours.
//         <outdir>/haplotype_coverage.csv  one row per selected haplotype: id,fraction as std::to_string prints it.
// --resolve RESIDUAL (with --assign only): RESIDUAL is the reference's residual_mutations.txt, one line
// `<pos><letter>,<v1>[,<v2>...]` per residual mutation (residual_file.hpp says what is refused).  The residual mutations
// are attributed to the selected haplotypes (arena::resolve_unaccounted_mutations, arena.cpp:698-904):
//         <outdir>/mutation_reads.csv      one row per residual mutation that a read carries: key,name,name,... -- key =
//                                          `<pos><letter>:<v1>:<v2>...`, then the names reverse_merge lists for the reads
//                                          that carry it, reads in input order.
//         <outdir>/mutation_haplotypes.csv one row per residual mutation with a read that carries it or holds an N at
//                                          its site: key,id,id,... -- the selected haplotypes its reads point to, in
//                                          the order of FILE.
//                                          The reference's row order in both files is that of a concurrent hash map and
//                                          not defined; here the rows follow RESIDUAL.
// --neighbors FILE [--radius R] [--max-neighbors L]: FILE names selected haplotypes in the format of --assign.  After
// the map every selected haplotype is expanded to its neighbours (arena::closest_neighbors, arena.cpp:171-207: the
// haplotypes within R mutations, default 2, reached through haplotypes within R; the L best, default 500, in the
// reference's order by score, leaf count and identifier -- config.hpp:24-25) and the lists are united ("add
// neighbors", post_filter.hpp:56-64): one round of the Freyja loop between two runs of --assign.
//         <outdir>/haplotype_neighbors.csv one row per selected haplotype, in the order of FILE: id,id:distance,... --
//                                          its neighbours (itself among them) in rank order with their distances.
//         <outdir>/next_selection.txt      the union in rank order, one identifier per line: the next FILE.
// --peaks [--top-n T] [--max-peaks P] [--peak-radius Q] (defaults 10, 300, 2: config.hpp:19-22): the whole of
// wepp_filter::filter (initial_filter.cpp:455-506) -- the map, the peak-removal loop and the five expansion rounds:
//         <outdir>/peaks.txt               the selection in the checkpoint format of pipeline::save: one arena index per
//                                          line, the peaks (ascending) then the neighbours (ascending).  --assign reads it.
//         <outdir>/peak_reads.csv          one row per peak in the order it was chosen: id,reads,degree,step -- the reads
//                                          the loop removed for it, the sum of their degrees, the step that chose it.
// --clade-idx N (with --assign only): the text behind the first tab or comma of every line of FILE is the haplotype's
// abundance (strtod; a missing or unparsable value is an error), and the selection is named by lineage from annotation
// column N of the MAT (arena::dump_haplotype_proportion / dump_lineage_proportion, arena.cpp:446-492, :530-588):
//         <outdir>/haplotype_proportion.csv  one row per selected haplotype in the order of FILE: id,lineage,abundance
//                                          (std::to_string).  The lineage is the first annotation on the way from the
//                                          first source node of the condensed node to the root, then "/" + annotation
//                                          for every further source node that is itself annotated (arena.cpp:462-483).
//         <outdir>/lineage_proportion.csv  one row per lineage: lineage,sum of its haplotypes' abundances, accumulated
//                                          in the order of FILE; rows by descending sum.  The reference's std::sort
//                                          compares the sums only and leaves ties in the order of its hash map: here
//                                          equal sums go by ascending name.
// N beyond the last column prints the reference's error line (arena.cpp:458): the lineage column stays empty and
// lineage_proportion.csv has no rows.  With --dump, --clade-idx prints `lineage <haplotype>\t<name>` for every haplotype.
// --uncertainty (with --assign only): arena::dump_haplotype_uncertainty (arena.cpp:494-528)
//         <outdir>/haplotype_uncertainty.csv one row per selected haplotype in the order of FILE: max_dist,id,id,... --
//                                          the nodes of the full tree that were merged into its condensed node (they
//                                          differ only at sites no read covers), in the order of node_mappings, and the
//                                          largest mutation distance between two of them: one wepp_geno_diameters call
//                                          for the whole selection.
// --haplotypes (with --assign only): arena::dump_haplotypes (arena.cpp:906-931)
//         <outdir>/haplotypes.tsv          one SAM-like row per selected haplotype in the order of FILE: id, 0, the first
//                                          token of the FASTA header, 1, 60, <len>M, *, 0, 0, the haplotype's sequence,
//                                          <len> x '?', MD:Z:..., RG:Z:group.  Host code, no kernel.
// --truth TRUE (with --assign only): arena::print_mutation_distance (arena.cpp:251-301) for simulated data.  TRUE holds
// one identifier of a node of the full tree per line (an unknown or repeated identifier is an error).  Printed to
// stdout: `--- ground truth <n> haps; predicted <k> haps`, per true node `* dist: %02d true_node: <id> pred_node: <id> `
// -- the least mutation distance to a selected haplotype, both genotypes restricted to the sites a read covers
// (site_read_map), and the first haplotype of FILE attaining it (wepp_geno_nearest) -- and `average mutation_distance: %0.3f`.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <unordered_set>

#include "../../include/wepp_place.h"
#include "haplotype_report.hpp"
#include "wepp_filter.hpp"

// dump_haplotype_uncertainty's distances (arena.cpp:503-516) in one wepp_geno_diameters call: max_dist[k] = the largest
// mutation_distance between the genotypes of two of node_mappings[selected[k]] (nodes of the full tree), 0 for one source
static int haplotype_uncertainty(const std::vector<MAT::Node*>& selected, const std::unordered_map<MAT::Node*, std::vector<MAT::Node*>>& node_mappings,
                                 std::vector<int>& max_dist, int device) {
    genotype_lister lister;
    packed_genotypes items;
    std::vector<uint32_t> grp_off{0};
    for (MAT::Node* hap : selected) {
        for (const MAT::Node* src : node_mappings.at(hap)) items.add(lister.get_mutations(src));
        grp_off.push_back(items.size());
    }
    const wepp_genotypes g{items.size(), items.item_off.data(), items.item_word.data()};
    std::vector<int32_t> diam(selected.size(), 0);
    if (wepp_geno_diameters(device, &g, nullptr, 0, (uint32_t)selected.size(), grp_off.data(), diam.data()) != WEPP_OK) {
        fprintf(stderr, "ERROR: %s\n", wepp_last_error());
        return 1;
    }
    max_dist.assign(diam.begin(), diam.end());
    return 0;
}

// print_mutation_distance's minima (arena.cpp:258-294) in one wepp_geno_nearest call: for every node of true_nodes the
// least mutation_distance to a node of `predicted` (full-tree nodes: the first source of every selected haplotype),
// both genotypes restricted to `sites`, and the first node of `predicted` attaining it
static int truth_distances(const std::vector<MAT::Node*>& true_nodes, const std::vector<MAT::Node*>& predicted, const std::unordered_set<int>& sites,
                           std::vector<int>& min_dist, std::vector<int>& nearest, int device) {
    genotype_lister lister;
    packed_genotypes items;
    for (const MAT::Node* n : true_nodes) items.add(lister.get_mutations(n));
    for (const MAT::Node* n : predicted) items.add(lister.get_mutations(n));
    uint32_t keep_positions = 0;
    const std::vector<uint32_t> keep = keep_bits_of(sites, &keep_positions);
    const uint32_t none = 0;                                              // (no site is covered: an empty mask, not "keep all")
    const wepp_genotypes g{items.size(), items.item_off.data(), items.item_word.data()};
    std::vector<int32_t> md(true_nodes.size(), 0);
    std::vector<uint32_t> nr(true_nodes.size(), 0);
    if (wepp_geno_nearest(device, &g, (uint32_t)true_nodes.size(), keep.empty() ? &none : keep.data(), keep_positions, md.data(), nr.data(), nullptr) !=
        WEPP_OK) {
        fprintf(stderr, "ERROR: %s\n", wepp_last_error());
        return 1;
    }
    min_dist.assign(md.begin(), md.end());
    nearest.assign(nr.begin(), nr.end());
    return 0;
}

int main(int argc, char** argv) {
    std::string mat_f, reads_f, ref_f, mask_f, assign_f, resolve_f, neighbors_f, truth_f, outdir = ".";
    bool want_uncertainty = false, want_haplotypes = false;
    int device = 0, radius = 2, max_neighbors = 500;       // config.hpp:24-25
    int clade_idx = -1;                                     // --clade-idx: -1 = not given
    peaks_params peak_par;
    bool dump = false, want_peaks = false;
    for (int i = 1; i < argc; i++) {
        auto need = [&](const char* flag) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", flag); exit(1); }
            return argv[++i];
        };
        if (!strcmp(argv[i], "-i")) mat_f = need("-i");
        else if (!strcmp(argv[i], "-r")) reads_f = need("-r");
        else if (!strcmp(argv[i], "-f")) ref_f = need("-f");
        else if (!strcmp(argv[i], "-m")) mask_f = need("-m");
        else if (!strcmp(argv[i], "-d")) outdir = need("-d");
        else if (!strcmp(argv[i], "--device")) device = atoi(need("--device"));
        else if (!strcmp(argv[i], "--dump")) dump = true;
        else if (!strcmp(argv[i], "--assign")) assign_f = need("--assign");
        else if (!strcmp(argv[i], "--resolve")) resolve_f = need("--resolve");
        else if (!strcmp(argv[i], "--neighbors")) neighbors_f = need("--neighbors");
        else if (!strcmp(argv[i], "--radius")) radius = atoi(need("--radius"));
        else if (!strcmp(argv[i], "--max-neighbors")) max_neighbors = atoi(need("--max-neighbors"));
        else if (!strcmp(argv[i], "--peaks")) want_peaks = true;
        else if (!strcmp(argv[i], "--uncertainty")) want_uncertainty = true;
        else if (!strcmp(argv[i], "--haplotypes")) want_haplotypes = true;
        else if (!strcmp(argv[i], "--truth")) truth_f = need("--truth");
        else if (!strcmp(argv[i], "--top-n")) peak_par.top_n = atoi(need("--top-n"));
        else if (!strcmp(argv[i], "--max-peaks")) peak_par.max_peaks = atoi(need("--max-peaks"));
        else if (!strcmp(argv[i], "--peak-radius")) peak_par.peak_radius = atoi(need("--peak-radius"));
        else if (!strcmp(argv[i], "--clade-idx")) {
            const char* v = need("--clade-idx");
            char* endp = nullptr;
            const long n = strtol(v, &endp, 10);
            if (endp == v || *endp != '\0' || n < 0 || n > 1000000) { fprintf(stderr, "ERROR: --clade-idx needs a column number (0, 1, ...), got '%s'\n", v); return 1; }
            clade_idx = (int)n;
        }
        else { fprintf(stderr, "usage: wepp-epp -i tree.pb -r reads.pb -f ref.fa [-m mask.bed] -d outdir [--device N] [--assign FILE [--resolve RESIDUAL]] [--neighbors FILE [--radius R] [--max-neighbors L]] [--peaks [--top-n T] [--max-peaks P] [--peak-radius Q]] [--clade-idx N] [--assign FILE [--uncertainty] [--haplotypes] [--truth TRUE]]\n"); return 1; }
    }
    if (mat_f.empty() || reads_f.empty() || ref_f.empty()) {
        fprintf(stderr, "usage: wepp-epp -i tree.pb -r reads.pb -f ref.fa [-m mask.bed] -d outdir [--device N] [--assign FILE [--resolve RESIDUAL]] [--neighbors FILE [--radius R] [--max-neighbors L]] [--peaks [--top-n T] [--max-peaks P] [--peak-radius Q]] [--clade-idx N] [--assign FILE [--uncertainty] [--haplotypes] [--truth TRUE]]\n");
        return 1;
    }
    if (!resolve_f.empty() && assign_f.empty()) {
        fprintf(stderr, "ERROR: --resolve needs --assign: residual mutations are attributed to the selected haplotypes\n");
        return 1;
    }
    if ((want_uncertainty || want_haplotypes || !truth_f.empty()) && assign_f.empty()) {
        fprintf(stderr, "ERROR: %s needs --assign: FILE names the selected haplotypes\n", want_uncertainty ? "--uncertainty" : want_haplotypes ? "--haplotypes" : "--truth");
        return 1;
    }
    if (clade_idx >= 0 && assign_f.empty() && !dump) {
        fprintf(stderr, "ERROR: --clade-idx needs --assign: FILE names the haplotypes and their abundances\n");
        return 1;
    }
    if (radius < 0 || max_neighbors < 1) {
        fprintf(stderr, "ERROR: --radius must be at least 0 and --max-neighbors at least 1\n");
        return 1;
    }
    if (peak_par.top_n < 1 || peak_par.max_peaks < 1 || peak_par.peak_radius < 0) {
        fprintf(stderr, "ERROR: --top-n and --max-peaks must be at least 1 and --peak-radius at least 0\n");
        return 1;
    }
    try {
        std::string reference = load_reference(ref_f);
        MAT::Tree T = MAT::load_mutation_annotated_tree(mat_f);
        T.uncondense_leaves();                                            // dataset.hpp:222
        std::unordered_map<std::string, std::vector<std::string>> reverse_merge;
        std::vector<raw_read> reads = load_reads_from_proto(reference, reads_f, reverse_merge);
        std::vector<int> mask = mask_f.empty() ? std::vector<int>() : load_masked_sites(mask_f);
        mask_reads(reads, mask);                                          // arena.hpp:60-72
        std::unordered_map<MAT::Node*, std::vector<MAT::Node*>> mappings;
        MAT::Tree condensed = create_condensed_tree(T.root, site_read_map(reads, mask), mappings);
        fprintf(stderr, "%zu reads, %zu nodes, %zu haplotypes after condensing\n", reads.size(), T.size(), condensed.size());
        // the lineage of a condensed node in annotation column clade_idx (arena.cpp:462-483)
        const int max_clades_idx = (int)T.get_num_annotations() - 1;
        auto lineage_of = [&](MAT::Node* hap) {
            std::string name;
            const std::vector<MAT::Node*>& sources = mappings[hap];
            if (sources.empty()) return name;
            auto own = [&](const MAT::Node* n) -> const std::string& {
                static const std::string none;
                return n->clade_annotations.size() > (size_t)clade_idx ? n->clade_annotations[(size_t)clade_idx] : none;
            };
            for (const MAT::Node* anc = sources.front(); anc; anc = anc->parent)
                if (!own(anc).empty()) { name = own(anc); break; }
            for (size_t i = 1; i < sources.size(); i++)
                if (!own(sources[i]).empty()) name += "/" + own(sources[i]);
            return name;
        };
        if (dump) {
            if (clade_idx >= 0 && clade_idx <= max_clades_idx)
                for (MAT::Node* n : condensed.depth_first_expansion()) printf("lineage %s\t%s\n", n->identifier.c_str(), lineage_of(n).c_str());
            for (auto& r : reads) {
                printf("read %s %d %d %d", r.read.c_str(), r.start, r.end, r.degree);
                for (auto& m : r.mutations) printf(" %d:%d:%d", m.position, (int)m.ref_nuc, (int)m.mut_nuc);
                printf("\n");
            }
            for (MAT::Node* n : condensed.depth_first_expansion()) {
                printf("hap %s %s %zu", n->identifier.c_str(), n->parent ? n->parent->identifier.c_str() : "-", mappings[n].size());
                for (auto& m : n->mutations) printf(" %d:%d:%d", m.position, (int)m.ref_nuc, (int)m.mut_nuc);
                printf("\n");
            }
            for (MAT::Node* n : T.depth_first_expansion())
                printf("node %s %s\n", n->identifier.c_str(), n->parent ? n->parent->identifier.c_str() : "-");
            return 0;
        }
        // the selections are checked before the device is touched
        auto read_selection = [&](const std::string& file, std::vector<MAT::Node*>& nodes, std::vector<std::string>& ids,
                                  std::vector<double>* abundance = nullptr) -> bool {
            std::ifstream in(file);
            if (!in.is_open()) { fprintf(stderr, "ERROR: cannot read %s\n", file.c_str()); return false; }
            std::unordered_set<MAT::Node*> seen;
            std::vector<MAT::Node*> arena;                                    // filled when a line is an arena index
            std::string line;
            while (std::getline(in, line)) {
                if (!line.empty() && line.back() == '\r') line.pop_back();
                const size_t cut = line.find_first_of("\t,");
                const std::string tail = cut == std::string::npos ? std::string() : line.substr(cut + 1);
                line = line.substr(0, cut);
                if (line.empty()) continue;
                if (abundance) {
                    char* endp = nullptr;
                    const double v = strtod(tail.c_str(), &endp);
                    if (endp == tail.c_str()) { fprintf(stderr, "ERROR: %s: no abundance behind %s (--clade-idx reads one per line)\n", file.c_str(), line.c_str()); return false; }
                    abundance->push_back(v);
                }
                MAT::Node* n = condensed.get_node(line);
                if (!n && line.size() <= 9 && line.find_first_not_of("0123456789") == std::string::npos) {
                    if (arena.empty()) arena = condensed.depth_first_expansion();   // arena::from_mat, arena.cpp:3-55
                    const size_t k = (size_t)atol(line.c_str());
                    if (k < arena.size()) { n = arena[k]; line = n->identifier; }
                }
                if (!n) { fprintf(stderr, "ERROR: %s: %s is not a haplotype of the condensed tree\n", file.c_str(), line.c_str()); return false; }
                if (!seen.insert(n).second) { fprintf(stderr, "ERROR: %s: %s is listed more than once\n", file.c_str(), line.c_str()); return false; }
                nodes.push_back(n);
                ids.push_back(line);
            }
            if (nodes.empty()) { fprintf(stderr, "ERROR: %s names no haplotype\n", file.c_str()); return false; }
            return true;
        };
        std::vector<MAT::Node*> selected, pivots;
        std::vector<std::string> selected_ids, pivot_ids;
        std::vector<double> abundance;
        if (!assign_f.empty() && !read_selection(assign_f, selected, selected_ids, clade_idx >= 0 ? &abundance : nullptr)) return 1;
        if (!neighbors_f.empty() && !read_selection(neighbors_f, pivots, pivot_ids)) return 1;
        // so are the true nodes
        std::vector<MAT::Node*> true_nodes;
        if (!truth_f.empty()) {
            std::ifstream in(truth_f);
            if (!in.is_open()) { fprintf(stderr, "ERROR: cannot read %s\n", truth_f.c_str()); return 1; }
            std::unordered_set<MAT::Node*> seen;
            std::string line;
            while (std::getline(in, line)) {
                if (!line.empty() && line.back() == '\r') line.pop_back();
                if (line.empty()) continue;
                MAT::Node* n = T.get_node(line);
                if (!n) { fprintf(stderr, "ERROR: %s: %s is not a node of the tree\n", truth_f.c_str(), line.c_str()); return 1; }
                if (!seen.insert(n).second) { fprintf(stderr, "ERROR: %s: %s is listed more than once\n", truth_f.c_str(), line.c_str()); return 1; }
                true_nodes.push_back(n);
            }
            if (true_nodes.empty()) { fprintf(stderr, "ERROR: %s names no node\n", truth_f.c_str()); return 1; }
        }
        const std::string ref_name = want_haplotypes ? load_reference_name(ref_f) : std::string();
        // so is the residual list
        std::vector<residual_mutation> residual;
        if (!resolve_f.empty()) residual = load_residual_mutations(resolve_f, reference);
        filter_result filtered;
        cartesian_map_result own_map;
        if (want_peaks) {
            if (wepp_filter_filter(condensed, reads, reference.size(), mappings, peak_par, filtered, device) != 0) return 1;
        } else if (cartesian_map(condensed, reads, reference.size(), own_map, device) != 0) return 1;
        cartesian_map_result& res = want_peaks ? filtered.loop.map : own_map;
        {
            // an arena index in a selection file means a place in this order
            std::vector<MAT::Node*> pre = condensed.depth_first_expansion();
            if (pre != res.haplotypes) { fprintf(stderr, "ERROR: the arena order is not the pre-order of the condensed tree\n"); return 1; }
        }
        FILE* f = fopen((outdir + "/haplotype_scores.tsv").c_str(), "w");
        if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
        fprintf(f, "haplotype\tscore\tdist_divergence\tsources\n");
        for (size_t k = 0; k < res.haplotypes.size(); k++)
            fprintf(f, "%s\t%.12g\t%.12g\t%zu\n", res.haplotypes[k]->identifier.c_str(), res.score[k],
                    res.dist_divergence[k], mappings[res.haplotypes[k]].size());
        fclose(f);
        f = fopen((outdir + "/read_placements.tsv").c_str(), "w");
        if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
        fprintf(f, "read\tstart\tend\tdegree\tparsimony\tepps\n");
        for (size_t r = 0; r < reads.size(); r++)
            fprintf(f, "%s\t%d\t%d\t%d\t%d\t%d\n", reads[r].read.c_str(), reads[r].start, reads[r].end, reads[r].degree,
                    res.max_parismony[r], res.parsimony_multiplicity[r]);
        fclose(f);
        if (want_peaks) {
            const peaks_result& pk = filtered.loop;
            f = fopen((outdir + "/peaks.txt").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (int h : filtered.selection) fprintf(f, "%d\n", h);
            fclose(f);
            f = fopen((outdir + "/peak_reads.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (size_t k = 0; k < pk.peaks.size(); k++)
                fprintf(f, "%s,%d,%lld,%d\n", res.haplotypes[(size_t)pk.peaks[k]]->identifier.c_str(), pk.peak_reads[k], pk.peak_degree[k], pk.peak_step[k]);
            fclose(f);
            fprintf(stderr, "%zu peaks in %d steps, %d reads remain, %zu neighbours (round %d)\n", pk.peaks.size(), pk.n_steps, pk.n_remaining,
                    filtered.neighbors.size(), filtered.round);
        }
        if (!selected.empty()) {
            read2haplotype_result asg;
            if (read2haplotype_mapping(condensed, reads, reference.size(), selected, asg, device) != 0) return 1;
            f = fopen((outdir + "/haplotype_reads.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (size_t k = 0; k < selected.size(); k++) {
                if (asg.reads[k].empty()) continue;
                std::string row = selected_ids[k];
                for (int r : asg.reads[k]) {
                    auto it = reverse_merge.find(reads[(size_t)r].read);       // arena.cpp:628
                    if (it != reverse_merge.end()) for (auto const& name : it->second) row += "," + name;
                }
                fprintf(f, "%s\n", row.c_str());
            }
            fclose(f);
            f = fopen((outdir + "/haplotype_coverage.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (size_t k = 0; k < selected.size(); k++)
                fprintf(f, "%s,%s\n", selected_ids[k].c_str(), std::to_string(asg.coverage[k]).c_str());   // arena.cpp:681-688
            fclose(f);
        }
        if (want_uncertainty) {
            std::vector<int> max_dist;
            if (haplotype_uncertainty(selected, mappings, max_dist, device) != 0) return 1;
            f = fopen((outdir + "/haplotype_uncertainty.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (size_t k = 0; k < selected.size(); k++) fputs(uncertainty_row(max_dist[k], mappings[selected[k]]).c_str(), f);
            fclose(f);
        }
        if (want_haplotypes) {
            f = fopen((outdir + "/haplotypes.tsv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            genotype_lister lister;
            for (MAT::Node* hap : selected)                                     // hap->id names the first source node (arena.cpp:915)
                fputs(haplotype_row(hap->identifier, ref_name, reference, lister.get_mutations(mappings[hap].front())).c_str(), f);
            fclose(f);
        }
        if (!true_nodes.empty()) {
            std::vector<MAT::Node*> predicted;
            for (MAT::Node* hap : selected) predicted.push_back(mappings[hap].front());
            std::vector<int> min_dist, nearest;
            if (truth_distances(true_nodes, predicted, site_read_map(reads, mask), min_dist, nearest, device) != 0) return 1;
            printf("--- ground truth %zu haps; predicted %zu haps\n", true_nodes.size(), selected.size());
            double average_dist = 0.0;
            for (size_t t = 0; t < true_nodes.size(); t++) {
                average_dist += (double)min_dist[t] / true_nodes.size();       // arena.cpp:296
                fputs(truth_row(min_dist[t], true_nodes[t]->identifier, selected[(size_t)nearest[t]]->identifier).c_str(), stdout);
            }
            printf("average mutation_distance: %0.3f\n", average_dist);
        }
        if (clade_idx >= 0 && !selected.empty()) {
            const bool in_range = clade_idx <= max_clades_idx;
            if (!in_range) fprintf(stderr, "\n\nERROR: CLADE_IDX = %d exceeds Max CLADE_IDX = %d in the MAT!!!\n\n", clade_idx, max_clades_idx);   // arena.cpp:458
            f = fopen((outdir + "/haplotype_proportion.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            std::vector<std::pair<std::string, double>> lineages;             // in order of first appearance: the sums add up in FILE order
            std::unordered_map<std::string, size_t> lineage_at;
            for (size_t k = 0; k < selected.size(); k++) {
                const std::string name = in_range ? lineage_of(selected[k]) : std::string();
                fprintf(f, "%s,%s,%s\n", selected_ids[k].c_str(), name.c_str(), std::to_string(abundance[k]).c_str());   // arena.cpp:488
                auto at = lineage_at.emplace(name, lineages.size());
                if (at.second) lineages.emplace_back(name, 0.0);
                lineages[at.first->second].second += abundance[k];
            }
            fclose(f);
            f = fopen((outdir + "/lineage_proportion.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            if (in_range) {
                std::sort(lineages.begin(), lineages.end(), [](const auto& a, const auto& b) {
                    return a.second > b.second || (a.second == b.second && a.first < b.first);
                });
                for (auto& l : lineages) fprintf(f, "%s,%s\n", l.first.c_str(), std::to_string(l.second).c_str());   // arena.cpp:580-585
            }
            fclose(f);
        }
        if (!resolve_f.empty()) {
            resolve_result rr;
            if (resolve_unaccounted_mutations(condensed, reads, reference.size(), selected, residual, rr, device) != 0) return 1;
            f = fopen((outdir + "/mutation_reads.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (size_t m = 0; m < residual.size(); m++) {
                if (rr.covered_reads[m].empty()) continue;
                std::string row = residual[m].key;
                for (int r : rr.covered_reads[m]) {
                    auto it = reverse_merge.find(reads[(size_t)r].read);       // arena.cpp:816
                    if (it != reverse_merge.end()) for (auto const& name : it->second) row += "," + name;
                }
                fprintf(f, "%s\n", row.c_str());
            }
            fclose(f);
            f = fopen((outdir + "/mutation_haplotypes.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (size_t m = 0; m < residual.size(); m++) {
                if (rr.covered_reads[m].empty() && rr.n_masked[m] == 0) continue;
                std::string row = residual[m].key;
                for (int k : rr.best[m]) row += "," + selected_ids[(size_t)k];       // arena.cpp:895-903
                fprintf(f, "%s\n", row.c_str());
            }
            fclose(f);
        }
        if (!pivots.empty()) {
            std::vector<haplotype_key> keys = haplotype_keys(res, haplotype_leaf_counts(res.haplotypes, mappings));
            neighbors_result nb;
            if (closest_neighbors(condensed, pivots, keys, radius, max_neighbors, nb, device) != 0) return 1;
            f = fopen((outdir + "/haplotype_neighbors.csv").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (size_t k = 0; k < pivots.size(); k++) {
                std::string row = pivot_ids[k];
                for (size_t j = 0; j < nb.neighbors[k].size(); j++)
                    row += "," + keys[(size_t)nb.neighbors[k][j]].id + ":" + std::to_string(nb.distance[k][j]);
                fprintf(f, "%s\n", row.c_str());
            }
            fclose(f);
            f = fopen((outdir + "/next_selection.txt").c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot write into %s\n", outdir.c_str()); return 1; }
            for (int h : nb.next_selection) fprintf(f, "%s\n", keys[(size_t)h].id.c_str());
            fclose(f);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
