// clades_host_ref.cpp -- a plain multi-threaded host restatement of usher_common.cpp:603-615 for tools/diag/clades_probe.py
// (built by the probe, not part of the product): per sample and annotation column, has_unique of every optimal node
// from the node's mutation list against the sample's (usher_mapper.cpp:191-262), a walk up the parents to the first
// annotated node, std::string clade names, std::sort, and the runs the -D writer prints.  The samples are dealt to the
// threads in chunks; the reference runs this loop on one thread per sample ("can be parallelized").
// Names are "L%07u" of the id, so that the string order is the id order and the result can be compared with the device's.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

namespace {
struct In {
    uint32_t N, R, C;
    const int32_t* parent; const uint32_t* mut_off; const int32_t* mut_pos; const uint8_t* mut_ref; const uint8_t* mut_mut;
    const uint8_t* is_leaf; const uint32_t* bfs2id;
    const uint32_t* read_off; const uint32_t* read_word; const uint32_t* best_bfs_j; const uint64_t* best_off; const uint32_t* best_nodes;
    const uint32_t* clade_id;   // [C][N] by node id
};

bool has_unique(const In& in, uint32_t node, uint32_t r) {
    if (in.parent[node] < 0) return false;
    bool unique = false;
    uint32_t k = in.read_off[r];
    const uint32_t kend = in.read_off[r + 1];
    for (uint32_t m = in.mut_off[node]; m < in.mut_off[node + 1]; m++) {
        if (in.mut_pos[m] < 0) return true;
        bool found = false, found_pos = false;
        for (; k < kend; k++) {
            const uint32_t w = in.read_word[k];
            const int32_t pos = (int32_t)(w & 0xFFFFFu);
            if (pos == in.mut_pos[m]) {
                found_pos = true;
                if ((w >> 28) & 1u) found = true;
                else if (((w >> 24) & 15u) & in.mut_mut[m]) { found = true; break; }
            }
            if (in.mut_pos[m] < pos) break;
        }
        if (!found && !(!found_pos && in.mut_mut[m] == in.mut_ref[m])) unique = true;
    }
    return unique;
}

std::string clade_of(const In& in, uint32_t c, int32_t node, bool include_self) {
    char buf[16];
    for (int32_t cur = include_self ? node : in.parent[node]; cur >= 0; cur = in.parent[cur]) {
        const uint32_t id = in.clade_id[(size_t)c * in.N + (uint32_t)cur];
        if (id) { snprintf(buf, sizeof buf, "L%07u", id); return buf; }
    }
    return "UNDEFINED";
}
}  // namespace

// out_best[C][R] ids (0 = UNDEFINED); per (column, read) segment s = c * R + r: out_runs[s] runs; the runs themselves are
// appended per thread and only counted (the probe compares best and the run counts, and times the whole)
extern "C" int clades_host_ref(uint32_t N, uint32_t R, uint32_t C, const int32_t* parent, const uint32_t* mut_off, const int32_t* mut_pos,
                               const uint8_t* mut_ref, const uint8_t* mut_mut, const uint8_t* is_leaf, const uint32_t* bfs2id,
                               const uint32_t* read_off, const uint32_t* read_word, const uint32_t* best_bfs_j, const uint64_t* best_off,
                               const uint32_t* best_nodes, const uint32_t* clade_id, uint32_t n_threads, uint32_t* out_best,
                               uint32_t* out_runs) {
    const In in{N, R, C, parent, mut_off, mut_pos, mut_ref, mut_mut, is_leaf, bfs2id, read_off, read_word, best_bfs_j, best_off, best_nodes, clade_id};
    std::atomic<uint32_t> next{0};
    auto work = [&]() {
        std::vector<uint8_t> include;
        std::vector<std::string> names;
        for (;;) {
            const uint32_t lo = next.fetch_add(16), hi = std::min(R, lo + 16);
            if (lo >= R) return;
            for (uint32_t r = lo; r < hi; r++) {
                const uint64_t p0 = in.best_off[r], p1 = in.best_off[r + 1];
                include.resize(p1 - p0);
                for (uint64_t p = p0; p < p1; p++) {
                    const uint32_t node = in.bfs2id[in.best_nodes[p]];
                    include[p - p0] = !in.is_leaf[node] && !has_unique(in, node, r);
                }
                for (uint32_t c = 0; c < C; c++) {
                    names.resize(p1 - p0);
                    std::string best;
                    for (uint64_t p = p0; p < p1; p++) {
                        names[p - p0] = clade_of(in, c, (int32_t)in.bfs2id[in.best_nodes[p]], include[p - p0]);
                        if (in.best_nodes[p] == in.best_bfs_j[r]) best = names[p - p0];
                    }
                    std::sort(names.begin(), names.end());
                    uint32_t runs = 0;
                    for (size_t i = 0; i < names.size(); i++) runs += (i == 0 || names[i] != names[i - 1]) ? 1 : 0;
                    out_best[(size_t)c * R + r] = (!best.empty() && best[0] == 'L') ? (uint32_t)std::stoul(best.substr(1)) : 0u;
                    out_runs[(size_t)c * R + r] = runs;
                }
            }
        }
    };
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < n_threads; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    return 0;
}
