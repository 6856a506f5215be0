// place_dev.hpp -- device-side helpers shared by the placement kernels (route_kernels.hip, sweep_kernels.hip,
// walk_kernels.hip, pass2_kernels.hip, seed_kernels.hip): the packed word fields, the closed form of mapper2_body's
// per-position costs, wave-wide reductions on DPP row shifts, and the per-read result record.
//
// What is computed: for every read, exactly what the two passes of the reference's per-sample loop leave behind
// (src/usher_common.cpp:386-446, each iteration being mapper2_body, src/usher_mapper.cpp:168-506): the minimum
// parsimony score over eligible nodes, the number of eligible nodes attaining it, and the winner under the
// (num_leaves, BFS index) tie-break.  The score of node n for read S is
//     score(n) = base(n) + c_S(parent(n)) + adj_S(n)
// where base(n) is read-independent, c_S is the read-dependent correction of the parent genotype and adj_S(n) is
// non-zero only when n itself mutates a position listed in S.  c_S changes only at "events": entering / leaving
// the subtree of a node that mutates a position of S.  Integer work only: no MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_mat.hpp"

namespace wepp {

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;

// ---- word field helpers ------------------------------------------------------
// tree / event word: pos:20 | ref idx:2 | par:4 | mut:4 | exit | leaf (flatmat.hpp)
// read word:         pos:20 | ref:4 | mut:4 | missing           (wepp_place.h)
__device__ __forceinline__ uint32_t w_pos(uint32_t w) { return w & 0xFFFFFu; }
__device__ __forceinline__ uint32_t tw_ref(uint32_t w) { return 1u << ((w >> 20) & 3u); }
__device__ __forceinline__ uint32_t tw_par(uint32_t w) { return (w >> 22) & 15u; }
__device__ __forceinline__ uint32_t tw_mut(uint32_t w) { return (w >> 26) & 15u; }
__device__ __forceinline__ uint32_t rw_ref(uint32_t w) { return (w >> 20) & 15u; }
__device__ __forceinline__ uint32_t rw_mut(uint32_t w) { return (w >> 24) & 15u; }
__device__ __forceinline__ uint32_t rw_missing(uint32_t w) { return (w >> 28) & 1u; }

// f(x) = cost of allele state x for the read entry `s` minus its cost for an
// empty read; x == 0 means "no mutation on the root path" (then the read is
// compared with ITS OWN ref_nuc, usher_mapper.cpp:302-305,342).
__device__ __forceinline__ int f_state(uint32_t x, uint32_t tref, uint32_t s) {
    int c0 = (x != 0 && x != tref) ? 1 : 0;                                   // usher_mapper.cpp:426-437
    int cs = rw_missing(s) ? 0 : (((rw_mut(s) & (x ? x : rw_ref(s))) == 0) ? 1 : 0);  // :295,314-320,342
    return cs - c0;
}
// change of c_S for the descendants of a node carrying tree word `w`
__device__ __forceinline__ int enter_delta(uint32_t w, uint32_t s) {
    return f_state(tw_mut(w), tw_ref(w), s) - f_state(tw_par(w), tw_ref(w), s);
}
// own-score / common-count adjustments of the node carrying `w`
// (usher_mapper.cpp:205-264: "common" test with the sample vs. without it)
__device__ __forceinline__ void own_adjust(uint32_t w, uint32_t s, int& adj_score, int& adj_common) {
    const uint32_t ref = tw_ref(w), par = tw_par(w), mut = tw_mut(w);
    const int static_common = (mut == ref) ? 1 : 0;
    const int static_sub = static_common ? ((par != 0 && par != ref) ? 1 : 0) : 0;
    int actual_common, actual_sub;
    if (rw_missing(s)) { actual_common = 1; actual_sub = 0; }                  // :210-212
    else {
        actual_common = ((rw_mut(s) & mut) != 0) ? 1 : 0;                       // :215
        actual_sub = actual_common ? (((rw_mut(s) & (par ? par : rw_ref(s))) == 0) ? 1 : 0) : 0;
    }
    adj_score += static_sub - actual_sub;
    adj_common += actual_common - static_common;
}

// wave-wide minimum, returned wave-uniform: four DPP row shifts leave the minimum of every row of
// 16 lanes in its last lane, four readlanes and scalar mins finish (no LDS permutes)
__device__ __forceinline__ int wave_min_i32(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(0x7FFFFFFF, v, 0x111, 0xF, 0xF, false));   // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(0x7FFFFFFF, v, 0x112, 0xF, 0xF, false));   // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(0x7FFFFFFF, v, 0x114, 0xF, 0xF, false));   // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(0x7FFFFFFF, v, 0x118, 0xF, 0xF, false));   // row_shr:8
    const int a = __builtin_amdgcn_readlane(v, 15), b = __builtin_amdgcn_readlane(v, 31);
    const int c = __builtin_amdgcn_readlane(v, 47), d = __builtin_amdgcn_readlane(v, 63);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x111, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x112, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x114, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x118, 0xF, 0xF, false));
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 15), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 47), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    return min(min(a, b), min(c, d));
}

// wave-wide sum, returned wave-uniform (the same DPP pattern)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 15) + (uint32_t)__builtin_amdgcn_readlane((int)v, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 47) + (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// wave-wide inclusive scans (sum / max of unsigned values), every lane its own result: four DPP row shifts scan the
// rows of 16 lanes, two row broadcasts (lane 15 -> next row, lane 31 -> rows 2 and 3) carry across the rows
__device__ __forceinline__ uint32_t wave_scan_add_u32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);   // row_bcast:15 into rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);   // row_bcast:31 into rows 2, 3
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false));
    return v;
}

// lower_bound over a position-sorted slice of read words; returns the entry
// with exactly `pos` or NONE.
template <typename SPtr>
__device__ __forceinline__ uint32_t find_entry(SPtr S, uint32_t off, uint32_t k, uint32_t pos) {
    uint32_t lo = 0, hi = k;
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        uint32_t p = w_pos(S[off + mid]);
        if (p < pos) lo = mid + 1; else hi = mid;
    }
    if (lo < k) {
        uint32_t s = S[off + lo];
        if (w_pos(s) == pos) return s;
    }
    return NONE;
}

// has_unique of the node with DFS index d for the read with entries read_word[so .. so + k), from the node's own
// mutation words (usher_mapper.cpp:184,199,262): the emitted flag of a read's winner, and the flag of every optimal
// node of a read in clades_kernels.hip
__device__ __forceinline__ uint32_t node_has_unique(const DevMAT& m, uint32_t d, const uint32_t* __restrict__ read_word,
                                                    uint32_t so, uint32_t k) {
    const uint32_t st = m.nstat[d];
    if (st & NS_ROOT_DEV) return 0u;
    if (st & NS_MASKED_DEV) return 1u;
    int ncom = (int)((st >> 14) & NS_CNT_MASK_DEV);
    int dummy = 0;
    for (uint32_t w = m.node_woff[d]; w < m.node_woff[d + 1]; w++) {
        const uint32_t tw = m.words[w];
        const uint32_t s = find_entry(read_word, so, k, w_pos(tw));
        if (s != NONE) own_adjust(tw, s, dummy, ncom);
    }
    return (ncom < (int)(st & NS_CNT_MASK_DEV)) ? 1u : 0u;
}

// the per-read outputs from a read's best (score, rank, count): the reference's BFS index of the winner and
// its has_unique flag recomputed from its own mutations (usher_mapper.cpp:472,492)
__device__ __forceinline__ void emit_result(const DevMAT& m, uint32_t r, const uint32_t* __restrict__ read_off,
                                            const uint32_t* __restrict__ read_word, int bs, uint32_t br, uint32_t cnt,
                                            uint32_t* __restrict__ best_bfs_j, int32_t* __restrict__ score,
                                            uint32_t* __restrict__ num_best, uint32_t* __restrict__ flags) {
    // the root always competes, so some chunk reports it or better; the clamp only keeps a broken
    // invariant from becoming an out-of-bounds read
    const uint32_t d = m.rank2dfs[br < m.N ? br : 0u];
    const uint32_t so = read_off[r];
    const uint32_t hu = node_has_unique(m, d, read_word, so, read_off[r + 1] - so);
    if (best_bfs_j) best_bfs_j[r] = m.dfs2bfs[d];
    if (score) score[r] = bs;
    if (num_best) num_best[r] = cnt;
    if (flags) flags[r] = hu ? WEPP_FLAG_HAS_UNIQUE_DEV : 0u;
}

// -----------------------------------------------------------------------------
// A read with MANY events at its positions: lane = list entry, no walk (the method: wave_kernels.hip).  The device code
// lives here because two units run it: k_walk_wave (wave_kernels.hip) and the wave-role workgroups of k_step
// (walk_kernels.hip), which are compiled separately.
// -----------------------------------------------------------------------------
constexpr uint32_t WW_R = WAVE_WALK_MAX_EVENTS / 64;      // rows of 64 entries of the largest read: entries per lane
constexpr int PK_BIAS = 2;
// LDS of a block of `waves` waves (words), for a read of more than 64 events (sorted_build below): the two sorted key
// arrays (64 bits a key), the entries' packed adjustments, their two prefix arrays in sorted order; behind them four
// words per wave for the block's combination of its waves' bests
constexpr uint32_t WW_SORT_WORDS = 7 * WAVE_WALK_MAX_EVENTS;
__host__ __device__ constexpr uint32_t ww_lds_words(uint32_t waves) { return WW_SORT_WORDS + 4 * waves; }

struct Cand {
    int bs;
    uint32_t br, cnt, hu;
};
__device__ __forceinline__ void cand_take(Cand& c, int sc, uint32_t rk, uint32_t kk, uint32_t hu) {
    if (sc < c.bs) { c.bs = sc; c.br = rk; c.cnt = kk; c.hu = hu; }
    else if (sc == c.bs) { c.cnt += kk; if (rk < c.br) { c.br = rk; c.hu = hu; } }
}

// best statically eligible node of the untouched nodes [pos, stop) of an arena slice whose running c_S is `c`: the
// sparse table's byte says whether anything there can reach the bound, then the exact aggregate (as in k_walk)
__device__ __forceinline__ void range_candidate(const DevWalk& ix, const WcInfo& wi, uint32_t pos, uint32_t stop, int c, Cand& best, uint32_t& bytes) {
    const uint32_t len = stop - pos;
    const uint32_t lvl = len > 1 ? 32u - (uint32_t)__builtin_clz(len - 1) : 0u;
    const uint32_t mn = ix.sp[(size_t)wi.sp_off + (size_t)lvl * wi.n + pos];
    bytes += 1;
    if (mn == SP_NONE || (mn < SP_CLAMP && (int)mn + c > best.bs)) return;
    const uint32_t last = stop - 1, ba = pos / RQ_BLK, bl = last / RQ_BLK;
    SegNode ag{SCORE_INF_DEV, 0xFFFFFFFFu, 0u, 0u};
    auto join = [&](const SegNode x) {
        if (x.base < ag.base) ag = x;
        else if (x.base == ag.base) { ag.cnt += x.cnt; if (x.rank < ag.rank) { ag.rank = x.rank; ag.hu = x.hu; } }
    };
    if (ba == bl) {
        bytes += 16;
        if (pos == ba * RQ_BLK) join(ix.rq_pre[wi.node_off + last]);
        else if (stop == wi.n || stop == (ba + 1) * RQ_BLK) join(ix.rq_suf[wi.node_off + pos]);
        else
            for (uint32_t i = pos; i < stop; i++) {
                const NodeRec x = ix.nrec[wi.node_off + i];
                if (x.nstat & NS_ELIG0_DEV) {
                    const uint32_t hu = (x.nstat & NS_ROOT_DEV) ? 0u : (x.nstat & NS_MASKED_DEV) ? 1u :
                                        (((x.nstat >> 14) & NS_CNT_MASK_DEV) < (x.nstat & NS_CNT_MASK_DEV) ? 1u : 0u);
                    join(SegNode{x.base, x.rank, 1u, hu});
                }
            }
    } else {
        const uint32_t lo = ba + 1, hi = bl - 1;
        const SegNode none{SCORE_INF_DEV, 0xFFFFFFFFu, 0u, 0u};
        const uint32_t L = lo < hi ? 31u - (uint32_t)__builtin_clz(lo ^ hi) : 0u;
        const SegNode* trow = ix.rq_dst + wi.dst_off + (size_t)L * wi.rq_blocks;
        const SegNode s1 = ix.rq_suf[wi.node_off + pos], s2 = ix.rq_pre[wi.node_off + last];
        const SegNode s3 = lo <= hi ? trow[lo] : none, s4 = lo < hi ? trow[hi] : none;
        join(s1); join(s2); join(s3); join(s4);
        bytes += 64;
    }
    if (ag.cnt && ag.base + c <= best.bs) cand_take(best, ag.base + c, ag.rank, ag.cnt, ag.hu);
}

// the lists of one read, as every wave that works on it sees them: lane j < k holds list j
struct ReadLists {
    uint32_t k, E, w, off, len, start;
    int c0;
};
__device__ __forceinline__ ReadLists read_lists(const DevMAT& m, const DevWalk& ix, const WcInfo& wi, uint32_t lane, uint32_t rd,
                                                const uint32_t* __restrict__ read_off, const uint32_t* __restrict__ read_word) {
    ReadLists L;
    const uint32_t so = read_off[rd];
    L.k = read_off[rd + 1] - so;                         // (k <= WALK16_K: k_route)
    L.w = lane < L.k ? read_word[so + lane] : 0u;
    L.off = L.len = 0;
    if (lane < L.k && w_pos(L.w) <= m.max_pos) {
        const uint32_t o0 = ix.ix_head[wi.head_off + w_pos(L.w)].off, o1 = ix.ix_head[wi.head_off + w_pos(L.w) + 1].off;
        L.off = o0;
        L.len = o1 - o0 - 1u;                            // (every list ends in a sentinel)
    }
    const uint32_t incl = wave_scan_add_u32(L.len);
    L.start = incl - L.len;
    L.E = min((uint32_t)__builtin_amdgcn_readlane((int)incl, 63), WAVE_WALK_MAX_EVENTS);   // (k_route admits no more)
    L.c0 = (int)__popcll(__ballot(lane < L.k && !rw_missing(L.w) && (rw_mut(L.w) & rw_ref(L.w)) == 0));
    return L;
}
// entry i of the concatenated lists: its place in the index and the read's word for its position
__device__ __forceinline__ void locate(const ReadLists& L, uint32_t i, uint32_t& e, uint32_t& sw) {
    e = NONE; sw = 0;
    for (uint32_t j = 0; j < L.k; j++) {
        const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)L.start, (int)j), lj = (uint32_t)__builtin_amdgcn_readlane((int)L.len, (int)j);
        const uint32_t oj = (uint32_t)__builtin_amdgcn_readlane((int)L.off, (int)j), wj = (uint32_t)__builtin_amdgcn_readlane((int)L.w, (int)j);
        if (i - sj < lj) { e = oj + (i - sj); sw = wj; }
    }
}
// the three adjustments of an entry (the delta -2 .. 2, the other two -1 .. 1), each biased by PK_BIAS in a byte of its
// own, and a one in the top byte: the sum over the <= 16 entries of one node (one per listed position) stays inside
__device__ __forceinline__ uint32_t pack_adjust(const IxEnt& ent, uint32_t sw) {
    int d = 0, adj = 0, dcom = 0;
    // descendants take the allele; the root also scores itself with it (usher_mapper.cpp:266-271)
    if (ent.end > ent.node + 1 || ent.node == 0) d = enter_delta(ent.word, sw);
    own_adjust(ent.word, sw, adj, dcom);
    return (uint32_t)(d + PK_BIAS) | (uint32_t)(adj + PK_BIAS) << 8 | (uint32_t)(dcom + PK_BIAS) << 16 | 1u << 24;
}

// What a sequential walk would know at every entry (n, e) of a read.  Subtrees nest, so:
//   cb  = the deltas of the entries whose subtree holds n strictly inside (nl < n < el);
//   T   = the packed sum over the entries of the same node (the lowest of them owns the node and its stretches);
//   the stretch of untouched descendants starts at n + 1 with c_S = cb + the node's own deltas and stops at the first
//   entry node or subtree end at or behind n + 1 (its own end at the latest: a leaf's stretch is empty): stopA nodes on;
//   the stretch behind the subtree starts at e with cB = the deltas of the subtrees that hold e strictly inside and
//   stops at the first entry node at or behind e, or subtree end behind e (stopB, in half nodes; >= 0x80000000: no
//   cut); of the entries that end at e the lowest owns it.
//   "Lower" compares the entries' indices in the read.
struct PairAcc {
    int cb, cB;
    uint32_t T, stopA, stopB, fl;      // fl bit 0: an entry of the same node with a lower index; bit 1: ... of the same subtree end
};
// One pair of the all-pairs pass: what entry l = (nl, el) with the packed adjustments pl adds to the knowledge of the
// entry (node, end); `lower`: l's index in the read is below the entry's own.  Differences wrap to huge values when the
// cut lies in front of the start, so plain minima do.  The one statement of the arithmetic: the 64-lane pass (wave_read),
// the group pass (group_read) and the CPU (tests/cxx/group_pass_emu.cpp) all call it.
__host__ __device__ __forceinline__ uint32_t pair_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ void pair_update(PairAcc& a, uint32_t node, uint32_t end, uint32_t nl, uint32_t el, uint32_t pl, bool lower) {
    const int dl = (int)(pl & 0xFFu) - PK_BIAS;
    const uint32_t nl1 = nl + 1u, span = el - nl1, sA = node + 1u, e2 = end << 1;
    if (dl != 0) {
        if (node - nl1 < span) a.cb += dl;
        if (end - nl1 < span) a.cB += dl;
    }
    const bool same = nl == node;
    a.T += same ? pl : 0u;
    a.fl |= (lower && same ? 1u : 0u) | (lower && el == end ? 2u : 0u);
    a.stopA = pair_min(a.stopA, pair_min(nl - sA, el - sA));
    a.stopB = pair_min(a.stopB, pair_min((nl << 1) - e2, (el << 1) - 1u - e2));       // (entry nodes at e cut, ends behind e cut)
}
// the pass of a GROUP of G lanes (one read): entry `own` = (node, end) of a read of E <= G entries against all of them.
// get(l, nl, el, pl) hands out entry l -- on the device an exchange that EVERY lane of the wave takes part in, whatever
// its own group's E, so only the update is guarded.
template <uint32_t G, typename Get>
__host__ __device__ __forceinline__ PairAcc group_pairs(uint32_t node, uint32_t end, uint32_t own, uint32_t E, Get get) {
    PairAcc a{0, 0, 0u, NONE, NONE, 0u};
#pragma unroll
    for (uint32_t ll = 0; ll < G; ll++) {
        uint32_t nl, el, pl;
        get(ll, nl, el, pl);
        if (ll < E) pair_update(a, node, end, nl, el, pl, ll < own);
    }
    return a;
}

// ---- a read of more than 64 events: sort and scan instead of all pairs ----
// Every field of PairAcc is a rank, a prefix sum or a successor query over the entries' node and end keys:
//   sum of dl over nl < x < el  =  sum of dl over nl < x  -  sum of dl over el <= x      (el <= x implies nl < x),
// so the workgroup sorts the keys (node, index) and (end, index) -- 64 bits: keys reach 2^25, the index breaks ties, and
// the lowest index of a run of equal keys is the run's first element; a padding entry has the key NONE and sorts behind
// every real one --, scans the deltas and the packed adjustments in both orders, and every entry asks six binary
// searches.  O(E log^2 E) compare-exchanges over the workgroup instead of E^2 pair evaluations on one wave.  Barriers and
// LDS only: tests/cxx runs this code lane by lane on the CPU.
// sorted_build: `key` holds (node << 8 | i) at i and (end << 8 | i) at N + i, `pk` the packed adjustments at i (0 for a
// padding entry), written by the caller; all T threads of the workgroup call it.  Leaves both halves of `key` sorted,
// ppk[p] = the wrapping sum of pk over the first p + 1 entries in node order, and pdl[p] = the sums of (dl + PK_BIAS)
// over the first p + 1 entries in node order (low half) and in end order (high half; at most 4 * 256 each).
template <uint32_t N, uint32_t T>
__device__ __forceinline__ void sorted_build(unsigned long long* key, const uint32_t* pk, uint32_t* ppk, uint32_t* pdl, uint32_t tid) {
    static_assert(N <= 256 && (N & (N - 1u)) == 0u, "the index is the low byte of a key; a bitonic network");
    constexpr uint32_t C = (N + T - 1u) / T;
    __syncthreads();
    // (the loops stay rolled: unrolled, the per-stage indices of all stages are hoisted and cost k_step 18 VGPRs)
#pragma unroll 1
    for (uint32_t k = 2; k <= N; k <<= 1)
#pragma unroll 1
        for (uint32_t j = k >> 1; j; j >>= 1) {
            // (compare-exchange q of the N of a stage: N / 2 in each half, partners differ in bit j, direction by bit k inside the half)
            for (uint32_t q = tid; q < N; q += T) {
                const uint32_t i = ((q & ~(j - 1u)) << 1) | (q & (j - 1u)), l = i | j;
                const unsigned long long a = key[i], b = key[l];
                if ((a > b) == (((i & (N - 1u)) & k) == 0u)) { key[i] = b; key[l] = a; }
            }
            __syncthreads();
        }
    for (uint32_t p = tid; p < N; p += T) {
        const unsigned long long ka = key[p], kb = key[N + p];
        const uint32_t pa = (uint32_t)(ka >> 8) != NONE ? pk[ka & 0xFFu] : 0u, pb = (uint32_t)(kb >> 8) != NONE ? pk[kb & 0xFFu] & 0xFFu : 0u;
        ppk[p] = pa;
        pdl[p] = (pa & 0xFFu) | pb << 16;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t d = 1; d < N; d <<= 1) {
        uint32_t x[C], y[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t p = tid + c * T;
            x[c] = y[c] = 0u;
            if (p < N && p >= d) { x[c] = ppk[p - d]; y[c] = pdl[p - d]; }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t p = tid + c * T;
            if (p < N && p >= d) { ppk[p] += x[c]; pdl[p] += y[c]; }
        }
        __syncthreads();
    }
}
// the rows of a read of R rows into `lds` (7 * 64 R words: 2 N keys, then pk, ppk, pdl), wave r % W of the W its row r, and
// sorted_build by all of them
template <uint32_t R, uint32_t W>
__device__ __forceinline__ void sorted_fill(uint32_t* lds, uint32_t lane, uint32_t wv, const uint32_t (&bnode)[R], const uint32_t (&bend)[R], const uint32_t (&bpk)[R]) {
    constexpr uint32_t N = 64 * R;
    unsigned long long* key = (unsigned long long*)lds;
    uint32_t* pk = lds + 4 * N;
#pragma unroll
    for (uint32_t r = 0; r < R; r++)
        if (r % W == wv) {
            const uint32_t i = lane + 64 * r;
            key[i] = (unsigned long long)bnode[r] << 8 | i;
            key[N + i] = (unsigned long long)bend[r] << 8 | i;
            pk[i] = bpk[r];
        }
    sorted_build<N, 64 * W>(key, pk, pk + N, pk + 2 * N, wv * 64 + lane);
}
// entry i = (node, end) of the read against what sorted_fill left in `lds`
template <uint32_t N>
__device__ __forceinline__ PairAcc sorted_query(const uint32_t* lds, uint32_t i, uint32_t node, uint32_t end) {
    const unsigned long long* key = (const unsigned long long*)lds;
    const uint32_t *ppk = lds + 5 * N, *pdl = lds + 6 * N;
    PairAcc a{0, 0, 0u, NONE, NONE, 0u};
    if (node == NONE) return a;
    // how many keys lie below x: node keys < n, <= n, end keys <= n; then node keys < e, end keys <= e, < e -- three searches in
    // step at a time (six in step cost the walkers of k_step a resident wave per SIMD in registers)
    const unsigned long long n0 = (unsigned long long)node << 8, e0 = (unsigned long long)end << 8;
    const unsigned long long x[6] = {n0, n0 + 256u, n0 + 256u, e0, e0 + 256u, e0};
    const uint32_t half[6] = {0u, 0u, N, 0u, N, N};
    uint32_t r[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t g = 0; g < 6; g += 3) {
#pragma unroll
        for (uint32_t s = N / 2; s; s >>= 1)
#pragma unroll
            for (uint32_t q = g; q < g + 3; q++) if (key[half[q] + r[q] + s - 1u] < x[q]) r[q] += s;
#pragma unroll
        for (uint32_t q = g; q < g + 3; q++) if (key[half[q] + r[q]] < x[q]) r[q]++;
    }
    auto dl_node = [&](uint32_t c) { return c ? (int)(pdl[c - 1u] & 0xFFFFu) - PK_BIAS * (int)c : 0; };
    auto dl_end = [&](uint32_t c) { return c ? (int)(pdl[c - 1u] >> 16) - PK_BIAS * (int)c : 0; };
    auto key_at = [&](uint32_t h, uint32_t c) { return c < N ? (uint32_t)(key[h + c] >> 8) : NONE; };
    a.cb = dl_node(r[0]) - dl_end(r[2]);
    a.cB = dl_node(r[3]) - dl_end(r[4]);
    a.T = (r[1] ? ppk[r[1] - 1u] : 0u) - (r[0] ? ppk[r[0] - 1u] : 0u);
    // (the entry itself is in both runs: r[0], r[5] < N)
    a.fl = ((uint32_t)(key[r[0]] & 0xFFu) != i ? 1u : 0u) | ((uint32_t)(key[N + r[5]] & 0xFFu) != i ? 2u : 0u);
    a.stopA = min(key_at(0u, r[1]), key_at(N, r[2])) - (node + 1u);
    const uint32_t na = key_at(0u, r[3]), eb = key_at(N, r[4]);      // (entry nodes at e cut, ends behind e cut)
    a.stopB = min(na != NONE ? (na - end) << 1 : NONE, eb != NONE ? ((eb - end) << 1) - 1u : NONE);
    return a;
}

// The work of ONE wave of a workgroup of W waves on one read of E <= 64 R entries: row r = the entries lane + 64 r.  A
// read of one row is a wave's own (R == 1): an all-pairs pass of register broadcasts.  A larger read is the
// workgroup's: wave r % W puts row r into LDS (`lds`, ww_lds_words), all waves sort and scan (sorted_build), then wave
// r % W asks for the entries of row r, scores their nodes and asks for their stretches.
template <uint32_t R, uint32_t W>
__device__ __forceinline__ void wave_read(const DevWalk& ix, const WcInfo& wi, uint32_t lane, uint32_t wv, const ReadLists& L, uint32_t* lds, Cand& best,
                                          uint32_t& bytes, uint32_t& wave_bytes) {
    constexpr uint32_t OWN = (R + W - 1) / W;      // rows a wave finishes
    const uint32_t E = L.E;
    const int c0 = L.c0;
    uint32_t bnode[R], bend[R], bpk[R];
    uint32_t orank[OWN], onst[OWN];
    int obase[OWN];
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t i = lane + 64 * r;
        bnode[r] = bend[r] = NONE; bpk[r] = 0;
        if (r % W == 0) { orank[r / W] = 0; onst[r / W] = 0; obase[r / W] = 0; }
        uint32_t e, sw;
        locate(L, i, e, sw);
        if (i < E && e != NONE) {
            const IxEnt ent = ix.ix_ent[e];
            bnode[r] = ent.node;
            bend[r] = ent.end;
            bpk[r] = pack_adjust(ent, sw);
            if (r % W == wv) {
                obase[r / W] = ent.base;
                orank[r / W] = wi.has_pre ? ent.rank & IX_RANK_MASK : ent.rank;
                onst[r / W] = ent.nstat;
            }
        }
    }
    // ---- all pairs (R == 1): pair_update above, entry ll broadcast from its lane
    auto pairs = [&]() -> PairAcc {
        const uint32_t node = bnode[0], end = bend[0];
        PairAcc a{0, 0, 0u, NONE, NONE, 0u};
        for (uint32_t ll = 0; ll < E; ll++) {
            const uint32_t nl = (uint32_t)__builtin_amdgcn_readlane((int)bnode[0], (int)ll), el = (uint32_t)__builtin_amdgcn_readlane((int)bend[0], (int)ll);
            const uint32_t pl = (uint32_t)__builtin_amdgcn_readlane((int)bpk[0], (int)ll);
            pair_update(a, node, end, nl, el, pl, ll < lane);
        }
        return a;
    };
    // ---- every lane: its node, its stretches ----
    auto finish = [&](uint32_t row, const PairAcc& a, int base, uint32_t rank, uint32_t nst) {
        uint32_t node = NONE, end = NONE;
#pragma unroll
        for (uint32_t r = 0; r < R; r++) if (r == row) { node = bnode[r]; end = bend[r]; }
        if (node != NONE) {
            const uint32_t sA = node + 1u;
            const uint32_t cnt = PK_BIAS * (a.T >> 24);
            const int dsumT = (int)(a.T & 0xFFu) - (int)cnt, adjT = (int)((a.T >> 8) & 0xFFu) - (int)cnt, dcomT = (int)((a.T >> 16) & 0xFFu) - (int)cnt;
            if (!(a.fl & 1u)) {
                const uint32_t nmut = nst & NS_CNT_MASK_DEV, ncom0 = (nst >> 14) & NS_CNT_MASK_DEV;
                const bool leaf = nst & NS_LEAF_DEV, masked = nst & NS_MASKED_DEV, root = nst & NS_ROOT_DEV;
                const int c = c0 + a.cb;
                if (root) { if (base + c + dsumT <= best.bs) cand_take(best, base + c + dsumT, rank, 1u, 0u); }
                else if (!masked) {
                    const int sc = base + c + adjT, ncom = (int)ncom0 + dcomT;
                    const bool elig = leaf ? (ncom > 0) : (ncom > 0 || ncom == (int)nmut);     // usher_mapper.cpp:455-456
                    if (elig && sc <= best.bs) cand_take(best, sc, rank, 1u, ncom < (int)nmut ? 1u : 0u);
                }
                const uint32_t eA = min(sA + a.stopA, wi.n);
                if (sA < eA) range_candidate(ix, wi, sA, eA, c0 + a.cb + dsumT, best, bytes);
            }
            if (!(a.fl & 2u)) {
                const uint32_t eB = a.stopB >= 0x80000000u ? wi.n : min(end + ((a.stopB + 1u) >> 1), wi.n);     // (no cut behind e: the keys are below 2 n)
                if (end < eB) range_candidate(ix, wi, end, eB, c0 + a.cB, best, bytes);
            }
        }
        if (row == 0) {
            // the stretch from node 0 on is nobody's: the first lane asks for it
            uint32_t first_node = bnode[0];
#pragma unroll
            for (uint32_t r = 1; r < R; r++) first_node = min(first_node, bnode[r]);
            first_node = wave_min_u32(first_node);
            if (lane == 0 && first_node != 0u && wi.n > 0) range_candidate(ix, wi, 0u, min(first_node, wi.n), c0, best, bytes);
        }
        // (the read's offsets, words, list heads and stream record once; a 32-byte index entry per list entry)
        wave_bytes += (row == 0 ? 8 + 12 * L.k + 80 + 16 : 0) + 32 * min(64u, E - 64 * row);
    };
    if constexpr (R == 1) {
        finish(0u, pairs(), obase[0], orank[0], onst[0]);
    } else {
        constexpr uint32_t N = 64 * R;
        sorted_fill<R, W>(lds, lane, wv, bnode, bend, bpk);
        const uint32_t rows = max((E + 63) / 64, 1u);
#pragma unroll
        for (uint32_t j = 0; j < OWN; j++) {
            const uint32_t row = wv + j * W;
            if (row >= rows) break;
            uint32_t node = NONE, end = NONE;
#pragma unroll
            for (uint32_t r = 0; r < R; r++) if (r == row) { node = bnode[r]; end = bend[r]; }
            finish(row, sorted_query<N>(lds, lane + 64 * row, node, end), obase[j], orank[j], onst[j]);
        }
    }
}

// The many-event reads of a call, by the waves of workgroup `blk` of `n_blk` workgroups of W waves that loop over the list:
// list[0 .. count[0]): reads with <= 64 events, a wave each; list[n_reads - count[1] .. n_reads), from the back: reads
// with more, all waves of a workgroup each, first.  `lds`: ww_lds_words(W) words.
template <uint32_t W>
__device__ __forceinline__ void wave_walk_body(const DevMAT& m, uint32_t* lds, uint32_t blk, uint32_t n_blk, const uint32_t* __restrict__ list,
                                               uint32_t n_small, uint32_t n_big, uint32_t n_reads,
                                               const uint32_t* __restrict__ read_off, const uint32_t* __restrict__ read_word,
                                               const int32_t* __restrict__ root_score, uint32_t* __restrict__ best_bfs_j,
                                               int32_t* __restrict__ score_out, uint32_t* __restrict__ num_best,
                                               uint32_t* __restrict__ flags, unsigned long long* __restrict__ work_counter,
                                               const uint32_t* __restrict__ wsid) {
    static_assert(7 * 64 * WW_R == WW_SORT_WORDS, "wave_read lays the sorted pass of the largest read out in WW_SORT_WORDS");
    uint32_t* part_w = lds + WW_SORT_WORDS;                    // [4][W]: score, total, rank, has_unique of every wave
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const DevWalk ix = m.walks[WC_SLOT];                 // the walk arena: every stream is a slice of it
    uint32_t bytes = 0, wave_bytes = 0;     // what the lanes / the wave as a whole asked memory for
    auto reduce = [&](const Cand& best, int& smin, uint32_t& total, uint32_t& rmin, bool& hu) {
        smin = wave_min_i32(best.cnt ? best.bs : 0x7FFFFFFF);
        const bool at = best.cnt && best.bs == smin;
        total = wave_sum_u32(at ? best.cnt : 0u);
        rmin = wave_min_u32(at ? best.br : 0xFFFFFFFFu);
        hu = __ballot(at && best.br == rmin && best.hu) != 0ull;
    };
    auto emit = [&](uint32_t rd, int smin, uint32_t total, uint32_t rmin, bool hu) {
        if (best_bfs_j) best_bfs_j[rd] = m.rank2bfs[rmin < m.N ? rmin : 0u];
        if (score_out) score_out[rd] = smin;
        if (num_best) num_best[rd] = total;
        if (flags) flags[rd] = hu ? WEPP_FLAG_HAS_UNIQUE_DEV : 0u;
    };
    for (uint32_t it = blk; it < n_big; it += n_blk) {
        const uint32_t rd = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[n_reads - 1u - it]);
        const WcInfo wi = m.wc_info[wsid[rd]];
        const ReadLists L = read_lists(m, ix, wi, lane, rd, read_off, read_word);
        Cand best{root_score[rd] + 1, 0xFFFFFFFFu, 0u, 0u};        // the root always competes: nothing worse can win or tie
        if (L.E <= 128) wave_read<2, W>(ix, wi, lane, wv, L, lds, best, bytes, wave_bytes);
        else wave_read<WW_R, W>(ix, wi, lane, wv, L, lds, best, bytes, wave_bytes);
        int smin; uint32_t total, rmin; bool hu;
        reduce(best, smin, total, rmin, hu);
        if (lane == 0) { part_w[wv] = (uint32_t)smin; part_w[W + wv] = total; part_w[2 * W + wv] = rmin; part_w[3 * W + wv] = hu ? 1u : 0u; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (uint32_t v = 1; v < W; v++) {
                const int sv = (int)part_w[v];
                const uint32_t tv = part_w[W + v], rv = part_w[2 * W + v];
                if (sv < smin) { smin = sv; total = tv; rmin = rv; hu = part_w[3 * W + v]; }
                else if (sv == smin && tv) { total += tv; if (rv < rmin) { rmin = rv; hu = part_w[3 * W + v]; } }
            }
            emit(rd, smin, total, rmin, hu);
        }
        __syncthreads();
    }
    // (the small reads are dealt from the END of the grid: the first workgroups hold the large ones)
    for (uint32_t it = n_blk * W - 1u - (blk * W + wv); it < n_small; it += n_blk * W) {
        const uint32_t rd = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[it]);
        const WcInfo wi = m.wc_info[wsid[rd]];
        const ReadLists L = read_lists(m, ix, wi, lane, rd, read_off, read_word);
        Cand best{root_score[rd] + 1, 0xFFFFFFFFu, 0u, 0u};
        wave_read<1, W>(ix, wi, lane, 0u, L, lds, best, bytes, wave_bytes);
        int smin; uint32_t total, rmin; bool hu;
        reduce(best, smin, total, rmin, hu);
        if (lane == 0) emit(rd, smin, total, rmin, hu);
    }
    wave_bytes += wave_sum_u32(bytes);
    if (work_counter && lane == 0 && wave_bytes)
        atomicAdd(work_counter + WALK_COUNTERS + ((blk * W + wv) & (WALK_COUNTERS - 1)), (unsigned long long)wave_bytes);
}

// -----------------------------------------------------------------------------
// A read with FEW events: the same pass (wave_read<1, W>) by a GROUP of G lanes, 64 / G reads a wave -- the plain walkers
// of k_step (walk_kernels.hip), whose walk lane = read is a chain of dependent loads per event and as long as the longest
// lane of its wave.  Group lane j is list j of the read (k <= WALK8_K <= G lists), then entry j of the concatenated
// lists (E <= G entries: k_route admits no more to the class).  The groups of a wave are different reads, of different
// crowns: every number of the read and its stream is a per-lane value, and every exchange is taken by all 64 lanes.
// (The exchanges are templates on their value's type: a host compiler that parses this header for the sorted pass alone
// never instantiates them.)
// -----------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T lane_get(T v, uint32_t src) { return __shfl(v, (int)src); }
// inclusive sum over the lanes of a group up to this one
template <uint32_t G, typename T> __device__ __forceinline__ T group_scan_add(T v, uint32_t gl) {
#pragma unroll
    for (uint32_t d = 1; d < G; d <<= 1) {
        const T o = __shfl_up(v, d, (int)G);
        if (gl >= d) v += o;
    }
    return v;
}
// group-wide minimum / sum, every lane of the group its result (the partners of a butterfly over G stay inside the group)
template <uint32_t G, typename T> __device__ __forceinline__ T group_min(T v) {
#pragma unroll
    for (uint32_t d = 1; d < G; d <<= 1) { const T o = __shfl_xor(v, (int)d); v = o < v ? o : v; }
    return v;
}
template <uint32_t G, typename T> __device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (uint32_t d = 1; d < G; d <<= 1) v += __shfl_xor(v, (int)d);
    return v;
}
// the lanes of this lane's group among a ballot
template <uint32_t G> __device__ __forceinline__ uint32_t group_bits(unsigned long long b, uint32_t gbase) { return (uint32_t)(b >> gbase) & ((1u << G) - 1u); }

// read `rd` (have: the group holds one) of the arena slice `wi`, by the G lanes of a group; all 64 lanes call.  The
// group's first lane writes the four results.
template <uint32_t G>
__device__ __forceinline__ void group_read(const DevMAT& m, const DevWalk& ix, uint32_t lane, bool have, uint32_t rd, const WcInfo& wi,
                                           const uint32_t* __restrict__ read_off, const uint32_t* __restrict__ read_word,
                                           const int32_t* __restrict__ root_score, uint32_t* __restrict__ best_bfs_j,
                                           int32_t* __restrict__ score_out, uint32_t* __restrict__ num_best,
                                           uint32_t* __restrict__ flags, uint32_t& bytes) {
    static_assert(G >= WALK8_K && G <= 16 && 64 % G == 0, "a lane per list of the read; the groups tile the wave");
    const uint32_t gl = lane % G, gbase = lane - gl;
    // ---- the read's lists: lane j < k holds list j (read_lists, per group) ----
    uint32_t so = 0, k = 0;
    // (k <= WALK8_K lists and, below, E <= G entries is k_route's invariant for the list this role reads -- route_kernels.hip,
    // classify: `events <= walk_max_events` and `k <= WALK8_K` make PLAN_WALK8, and capi.cpp launches this G only for a walk
    // limit <= G.  The two clamps keep a broken invariant inside the group's lanes and the index's lists: the placement
    // would then be WRONG without a sign, so whoever changes the classes or the limit must keep both bounds.)
    if (have) { so = read_off[rd]; k = min(read_off[rd + 1] - so, WALK8_K); }
    const uint32_t w = gl < k ? read_word[so + gl] : 0u;
    uint32_t off = 0, len = 0;
    if (gl < k && w_pos(w) <= m.max_pos) {
        const uint32_t o0 = ix.ix_head[wi.head_off + w_pos(w)].off, o1 = ix.ix_head[wi.head_off + w_pos(w) + 1].off;
        off = o0;
        len = o1 - o0 - 1u;                              // (every list ends in a sentinel)
    }
    const uint32_t incl = group_scan_add<G>(len, gl), start = incl - len;
    const uint32_t E = min(lane_get(incl, gbase + G - 1u), G);                   // (the invariant above: the clamp never binds)
    const int c0 = (int)__popc(group_bits<G>(__ballot(gl < k && !rw_missing(w) && (rw_mut(w) & rw_ref(w)) == 0), gbase));
    // ---- entry gl of the concatenated lists (locate): the list that holds it, then that list's offset and read word ----
    uint32_t jsel = 0, isub = NONE;
#pragma unroll
    for (uint32_t j = 0; j < WALK8_K; j++) {
        const uint32_t sj = lane_get(start, gbase + j), lj = lane_get(len, gbase + j);
        if (gl - sj < lj) { jsel = j; isub = gl - sj; }
    }
    const uint32_t oj = lane_get(off, gbase + jsel), wj = lane_get(w, gbase + jsel);
    uint32_t node = NONE, end = NONE, pk = 0u, rank = 0u, nst = 0u;
    int base = 0;
    if (gl < E && isub != NONE) {
        const IxEnt ent = ix.ix_ent[oj + isub];
        node = ent.node;
        end = ent.end;
        pk = pack_adjust(ent, wj);
        base = ent.base;
        rank = wi.has_pre ? ent.rank & IX_RANK_MASK : ent.rank;
        nst = ent.nstat;
    }
    // ---- what a sequential walk would know at the entry: G exchanges instead of 64 broadcasts ----
    const PairAcc a = group_pairs<G>(node, end, gl, E, [&](uint32_t ll, uint32_t& nl, uint32_t& el, uint32_t& pl) {
        nl = lane_get(node, gbase + ll);
        el = lane_get(end, gbase + ll);
        pl = lane_get(pk, gbase + ll);
    });
    // ---- every lane: its node, its stretches (as wave_read's finish) ----
    Cand best{(have ? root_score[rd] : 0) + 1, 0xFFFFFFFFu, 0u, 0u};        // the root always competes: nothing worse can win or tie
    if (node != NONE) {
        const uint32_t sA = node + 1u;
        const uint32_t cnt = PK_BIAS * (a.T >> 24);
        const int dsumT = (int)(a.T & 0xFFu) - (int)cnt, adjT = (int)((a.T >> 8) & 0xFFu) - (int)cnt, dcomT = (int)((a.T >> 16) & 0xFFu) - (int)cnt;
        if (!(a.fl & 1u)) {
            const uint32_t nmut = nst & NS_CNT_MASK_DEV, ncom0 = (nst >> 14) & NS_CNT_MASK_DEV;
            const bool leaf = nst & NS_LEAF_DEV, masked = nst & NS_MASKED_DEV, root = nst & NS_ROOT_DEV;
            const int c = c0 + a.cb;
            if (root) { if (base + c + dsumT <= best.bs) cand_take(best, base + c + dsumT, rank, 1u, 0u); }
            else if (!masked) {
                const int sc = base + c + adjT, ncom = (int)ncom0 + dcomT;
                const bool elig = leaf ? (ncom > 0) : (ncom > 0 || ncom == (int)nmut);     // usher_mapper.cpp:455-456
                if (elig && sc <= best.bs) cand_take(best, sc, rank, 1u, ncom < (int)nmut ? 1u : 0u);
            }
            const uint32_t eA = min(sA + a.stopA, wi.n);
            if (sA < eA) range_candidate(ix, wi, sA, eA, c0 + a.cb + dsumT, best, bytes);
        }
        if (!(a.fl & 2u)) {
            const uint32_t eB = a.stopB >= 0x80000000u ? wi.n : min(end + ((a.stopB + 1u) >> 1), wi.n);     // (no cut behind e: the keys are below 2 n)
            if (end < eB) range_candidate(ix, wi, end, eB, c0 + a.cB, best, bytes);
        }
    }
    // the stretch from node 0 on is nobody's: the group's first lane asks for it
    const uint32_t first_node = group_min<G>(node);
    if (have && gl == 0 && first_node != 0u && wi.n > 0) range_candidate(ix, wi, 0u, min(first_node, wi.n), c0, best, bytes);
    // ---- the group's best ----
    const int smin = group_min<G>(best.cnt ? best.bs : 0x7FFFFFFF);
    const bool at = best.cnt && best.bs == smin;
    const uint32_t total = group_sum<G>(at ? best.cnt : 0u);
    const uint32_t rmin = group_min<G>(at ? best.br : 0xFFFFFFFFu);
    const bool hu = group_bits<G>(__ballot(at && best.br == rmin && best.hu), gbase) != 0u;
    if (have && gl == 0) {
        if (best_bfs_j) best_bfs_j[rd] = m.rank2bfs[rmin < m.N ? rmin : 0u];
        if (score_out) score_out[rd] = smin;
        if (num_best) num_best[rd] = total;
        if (flags) flags[rd] = hu ? WEPP_FLAG_HAS_UNIQUE_DEV : 0u;
        // (as the wave pass counts: list entry, stream record, the read's offsets, words and list heads, root score, rank
        // -> BFS index and results once; a 32-byte index entry per list entry)
        bytes += 4 + 64 + 8 + 12 * k + 4 + 4 + 16 + 32 * E;
    }
}

}  // namespace

}  // namespace wepp
