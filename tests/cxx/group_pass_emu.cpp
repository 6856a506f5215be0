// group_pass_emu.cpp -- the per-pair update that the 64-lane pass and the group pass of place_dev.hpp share (pair_update,
// and group_pairs: the loop of a group of G lanes around it) run on the CPU for G = 8 and 16, against what the sorted
// pass (sorted_fill / sorted_build / sorted_query, one host thread per lane on tests/cxx/hip_emu) gives for the same
// entries.  A program of its own (tests/test_group_pass_emulation.py builds it plain and with sanitizers): entry sets of
// 1 - 16 entries, random nestings with several entries on one node, shared subtree ends and entry nodes at other entries'
// ends, and the hand-made shapes of tests/sorted_pass_model.py.  Every PairAcc field must be bit for bit equal, except
// that stopB without a cut is NONE from the sorted pass and some wrapped difference >= 2^31 from the pairs.
// The wave intrinsics of the code around it are declared here so that the header parses, and end the run if called.
#include <stdio.h>
#include <stdlib.h>
#include <hip/hip_runtime.h>
inline int __builtin_amdgcn_update_dpp(int, int, int, int, int, bool) { abort(); }
inline int __builtin_amdgcn_readlane(int, int) { abort(); }
#include "../../wepp_amd/csrc/place_dev.hpp"
#include <random>
#include <string>
thread_local dim3 threadIdx, blockIdx; dim3 blockDim, gridDim; EmuBlock* g_blk;
alignas(16) unsigned char g_emu_lds[65536];
using namespace wepp;
namespace {
constexpr uint32_t SLOTS = 128, MAX_E = 16;      // (the smallest sorted pass the kernels instantiate: two rows of 64)
struct Ent { uint32_t node, end, pk; };
struct Case { std::string name; std::vector<Ent> e; };

// the sets [n][SLOTS] x (node, end, pk), padded with (NONE, NONE, 0), through one workgroup of two waves in turn
void k_sorted(const uint32_t* node, const uint32_t* end, const uint32_t* pk, const uint32_t* E, uint32_t n, uint32_t* out) {
    HIP_DYNAMIC_SHARED(uint32_t, lds)
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t c = 0; c < n; c++) {
        const size_t o = (size_t)c * SLOTS;
        uint32_t bnode[2], bend[2], bpk[2];
        for (uint32_t r = 0; r < 2; r++) { const uint32_t i = lane + 64 * r; bnode[r] = node[o + i]; bend[r] = end[o + i]; bpk[r] = pk[o + i]; }
        sorted_fill<2, 2>(lds, lane, wv, bnode, bend, bpk);
        if (wv == 0 && lane < E[c]) {
            const PairAcc a = sorted_query<SLOTS>(lds, lane, bnode[0], bend[0]);
            uint32_t* q = out + 6 * (o + lane);
            q[0] = (uint32_t)a.cb; q[1] = (uint32_t)a.cB; q[2] = a.T; q[3] = a.stopA; q[4] = a.stopB; q[5] = a.fl;
        }
        __syncthreads();
        __syncthreads();
    }
}

std::mt19937 rng(13);
uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }
uint32_t rand_pk() { return (below(5)) | (1u + below(3)) << 8 | (1u + below(3)) << 16 | 1u << 24; }      // (pack_adjust: delta -2 .. 2, the others -1 .. 1, biased by PK_BIAS)
// E entries on the nodes of a random tree of n nodes in preorder, nodes drawn with repetition
std::vector<Ent> random_tree(uint32_t E, uint32_t n, bool leaves_only) {
    std::vector<int> par(n, -1);
    for (uint32_t v = 1; v < n; v++) {
        int p = (int)v - 1;
        for (uint32_t s = below(4); s && par[p] >= 0; s--) p = par[p];
        par[v] = p;
    }
    std::vector<uint32_t> end(n), pool;
    for (uint32_t v = 0; v < n; v++) end[v] = v + 1;
    for (uint32_t v = n - 1; v > 0; v--) end[par[v]] = std::max(end[par[v]], end[v]);
    for (uint32_t v = 0; v < n; v++) if (!leaves_only || end[v] == v + 1) pool.push_back(v);
    std::vector<Ent> e;
    for (uint32_t i = 0; i < E; i++) { const uint32_t v = pool[below((uint32_t)pool.size())]; e.push_back({v, end[v], rand_pk()}); }
    return e;
}
std::vector<Case> make_cases() {
    std::vector<Case> cs;
    for (uint32_t E = 1; E <= MAX_E; E++) {
        const std::string s = ", E=" + std::to_string(E);
        for (uint32_t rep = 0; rep < 6; rep++) cs.push_back({"random tree" + s, random_tree(E, std::max(2u, E / 2 + 3 * rep), false)});
        cs.push_back({"leaves only" + s, random_tree(E, 3 * E + 2, true)});
        std::vector<Ent> one, ends, chain, root = random_tree(E, std::max(2u, E), false), top;
        for (uint32_t i = 0; i < E; i++) {
            one.push_back({5u, 9u, rand_pk()});
            ends.push_back({below(400), 400u, rand_pk()});
            const uint32_t v = below(std::max(1u, E / 3));
            chain.push_back({3 * v, 3 * v + 3, rand_pk()});          // (0,3) (3,6) ...: every node at the end of the entry before it
            top.push_back({(1u << 25) - 2u - below(40), (1u << 25) - 1u, rand_pk()});
        }
        root[below(E)] = {0u, std::max(2u, E), rand_pk()};
        top[0] = {0u, (1u << 25) - 1u, rand_pk()};
        cs.push_back({"one node" + s, one});
        cs.push_back({"all ends equal" + s, ends});
        cs.push_back({"node == end chains" + s, chain});
        cs.push_back({"the root entry" + s, root});
        cs.push_back({"keys at 2^25 - 1" + s, top});
    }
    return cs;
}

template <uint32_t G>
uint32_t check(const Case& c, const uint32_t* want) {
    const uint32_t E = (uint32_t)c.e.size();
    if (E > G) return 0;
    // a group's lanes: the entries, padded as group_read pads the lanes behind E
    Ent lanes[G];
    for (uint32_t l = 0; l < G; l++) lanes[l] = l < E ? c.e[l] : Ent{NONE, NONE, 0u};
    uint32_t bad = 0;
    for (uint32_t i = 0; i < E; i++) {
        const PairAcc a = group_pairs<G>(lanes[i].node, lanes[i].end, i, E, [&](uint32_t ll, uint32_t& nl, uint32_t& el, uint32_t& pl) {
            nl = lanes[ll].node; el = lanes[ll].end; pl = lanes[ll].pk;
        });
        const uint32_t got[6] = {(uint32_t)a.cb, (uint32_t)a.cB, a.T, a.stopA, a.stopB, a.fl};
        static const char* const field[6] = {"cb", "cB", "T", "stopA", "stopB", "fl"};
        for (uint32_t f = 0; f < 6; f++) {
            const uint32_t x = want[6 * i + f];
            const bool same = got[f] == x || (f == 4 && x == NONE && got[f] >= 0x80000000u);
            if (!same) { printf("G=%u, %s: entry %u: %s is %u from the pairs, %u from the sorted pass\n", G, c.name.c_str(), i, field[f], got[f], x); bad++; }
        }
    }
    return bad;
}
}  // namespace

int main() {
    static_assert(ww_lds_words(2) * 4 <= sizeof(g_emu_lds), "LDS of the emulation");
    const std::vector<Case> cs = make_cases();
    const uint32_t n = (uint32_t)cs.size();
    std::vector<uint32_t> node((size_t)n * SLOTS, NONE), end((size_t)n * SLOTS, NONE), pk((size_t)n * SLOTS, 0u), E(n), out((size_t)n * SLOTS * 6, 0u);
    for (uint32_t c = 0; c < n; c++) {
        E[c] = (uint32_t)cs[c].e.size();
        for (uint32_t i = 0; i < E[c]; i++) { node[c * SLOTS + i] = cs[c].e[i].node; end[c * SLOTS + i] = cs[c].e[i].end; pk[c * SLOTS + i] = cs[c].e[i].pk; }
    }
    memset(g_emu_lds, 0xA5, sizeof(g_emu_lds));
    emu_launch(k_sorted, dim3(1), dim3(128), (const uint32_t*)node.data(), (const uint32_t*)end.data(), (const uint32_t*)pk.data(), (const uint32_t*)E.data(), n, out.data());
    uint32_t bad = 0, ran8 = 0, ran16 = 0, shared_node = 0, shared_end = 0, node_at_end = 0, no_cut = 0;
    for (uint32_t c = 0; c < n; c++) {
        const uint32_t* want = out.data() + (size_t)c * SLOTS * 6;
        bad += check<8>(cs[c], want) + check<16>(cs[c], want);
        ran8 += E[c] <= 8; ran16++;
        for (uint32_t i = 0; i < E[c]; i++) {
            no_cut += want[6 * i + 4] == NONE;
            for (uint32_t l = 0; l < i; l++) {
                shared_node += cs[c].e[i].node == cs[c].e[l].node;
                shared_end += cs[c].e[i].end == cs[c].e[l].end && cs[c].e[i].node != cs[c].e[l].node;
                node_at_end += cs[c].e[i].node == cs[c].e[l].end || cs[c].e[l].node == cs[c].e[i].end;
            }
        }
    }
    printf("sets=%u g8=%u g16=%u shared_node=%u shared_end=%u node_at_end=%u no_cut=%u mismatches=%u\n", n, ran8, ran16, shared_node, shared_end, node_at_end, no_cut, bad);
    // (the sets must hold the shapes the comparison is about)
    if (!shared_node || !shared_end || !node_at_end || !no_cut) { printf("the entry sets miss a shape\n"); return 2; }
    return bad ? 1 : 0;
}
