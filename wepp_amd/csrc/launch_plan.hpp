// launch_plan.hpp -- what a placement call launches behind its routing counters, as a pure function of the counters
// (capi.cpp: place_device calls it once the host has them; tests/cxx/launch_plan_main.cpp runs it without a GPU).
// The planner sees no device address: a list is its offset into the call's grouped read list, and of a stream it reads
// the three numbers of its geometry (NB, ncp, cp_stride) and the bytes of one sweep; of DevMAT bm_words, max_pos,
// n_streams, seed_chunks and wc_windows.  The launch functions of capi.cpp turn offsets into pointers.
#pragma once
#include <algorithm>
#include <cstdio>

#include "../../include/wepp_place.h"
#include "device_mat.hpp"
#include "errors.hpp"

namespace wepp {

// one tile plan: the reads of a plan id that sweep a stream in tiles
struct TilePlan {
    uint32_t t, sid;                 // stream as the `[plan]` line names it (a window stream is the whole tree for its reads); index among the streams / window streams
    uint32_t count, off, T, ntiles, nchunks, bpc, NB, ncp, ent_cap, key_cap, lds_bytes;
    bool s_in_lds, dense, window, win_table;
    size_t part_off;
    uint64_t sbytes;
    const uint32_t* lst;             // left null here, like WalkPlanDev::list: the launch side's pointer to the plan's reads
};

struct LaunchPlan {
    TilePlan plans[MAX_PLANS];
    // the partition of the tile plans, each part in launch order: fused into one launch (longest chunks first), the
    // table window plans (one launch, longest chunks first), launched on their own
    uint32_t np, order[MAX_PLANS], n_plain, wins[MAX_WINDOWS], n_wins, others[MAX_PLANS], n_other;
    // walk plans (device_mat.hpp): the reads of one (class, stream) that walk their own events; the class's
    // list begins at info[TI_OFF + plan_id(cls, 0)]
    WalkPlans walkc[2];
    uint32_t walkc_reads[2];
    uint64_t n_jobs[2], walk_reads;  // walk_reads: reads of the call that walk, whoever launches them
    uint32_t arena_n, arena_off, arena_maxk, seed_n, seed_off, seed_maxk;
    size_t arena_part, part_total;   // part_total: bytes of the tile plans' and the arena's partials
    uint64_t passes, bytes;          // the call's statistics
};

// Who reads the grouped read list: a plan with reads is a consumer unless its class is placed out of k_route's own
// tables: the plain walk classes always, a chunked class that fitted its blind tables (TI_JOVER == 0: launched blind or
// from the counters, never by a plan of the host).
inline bool lists_needed(const uint32_t* info) {
    for (uint32_t id = 0; id < MAX_PLANS; id++) {
        if (!info[TI_COUNT + id]) continue;
        const uint32_t cls = plan_class(id);
        if (cls == PLAN_WALK8 || cls == PLAN_WALK16) continue;
        if ((cls == PLAN_WALKC8 || cls == PLAN_WALKC16) && !info[TI_JOVER + (cls - PLAN_WALKC8)]) continue;
        return true;
    }
    return false;
}

// the tile rule.  Reads per tile: at most MAX_TILE_ENTRIES read words per tile (long reads share a sweep between
// fewer reads), a power of two, never more than the knob; long reads take the dense (table) variant of the sweep
inline uint32_t tile_reads(uint32_t T, uint32_t maxk) { while (T > 1 && (uint64_t)T * maxk > MAX_TILE_ENTRIES) T >>= 1; return T; }
inline bool takes_table(uint32_t maxk, uint32_t max_pos) { return maxk <= MAX_TILE_ENTRIES && maxk >= DENSE_MIN_READ_WORDS && max_pos < DENSE_MAX_POS; }

// the tile plan of `count` reads of at most maxk words on stream st of sbytes bytes (win_tiles: the tiles of all table
// window plans of the call when they share a launch, else 0); p.t, p.sid, p.off and p.window are the caller's
inline void plan_tiles(TilePlan& p, uint32_t count, uint32_t maxk, uint32_t T, const DevStream& st, uint64_t sbytes, const DevMAT& m, uint64_t win_tiles) {
    p.sbytes = sbytes;
    p.NB = st.NB;
    p.ncp = st.ncp;
    p.count = count;
    const uint32_t Tp = p.T = tile_reads(T, maxk);
    p.ntiles = (count + Tp - 1) / Tp;
    // a read longer than MAX_TILE_ENTRIES words is swept alone with its words left in global memory
    p.s_in_lds = maxk <= MAX_TILE_ENTRIES;
    p.dense = takes_table(maxk, m.max_pos);
    const uint64_t need = std::min<uint64_t>((uint64_t)std::min(Tp, count) * maxk, MAX_TILE_ENTRIES);
    const uint32_t cap = (uint32_t)((need + 63) & ~63ull);
    uint32_t kcap = 64;
    while (kcap < need) kcap <<= 1;                        // the bitonic network wants a power of two
    p.ent_cap = p.s_in_lds ? cap : 0;
    p.key_cap = p.dense ? kcap : 0;
    // long reads inside a window: per-position read masks instead of sorted keys (the argument then
    // carries the window's first position)
    p.win_table = p.window && p.dense;
    if (p.win_table) p.key_cap = p.sid * WIN_STRIDE;
    p.lds_bytes = p.s_in_lds ? sweep_lds_bytes(m.bm_words, cap, kcap, p.dense, p.win_table) : m.bm_words * 4;
    // chunks: enough single-wave workgroups to fill 256 CUs, cut at checkpoints
    uint32_t nchunks = std::max<uint32_t>(1, ((p.dense ? SWEEP_TARGET_WAVES_DENSE : SWEEP_TARGET_WAVES) + p.ntiles - 1) / p.ntiles);
    if (p.win_table && win_tiles) nchunks = std::max<uint32_t>(1, (uint32_t)((SWEEP_TARGET_WAVES_DENSE + win_tiles - 1) / win_tiles));
    // ... and chunks no longer than what stays in an XCD's L2 while the tiles sweep it: the waves of
    // a launch are ordered chunk-major (all tiles of chunk 0, then of chunk 1, ...), so the ~4 K
    // resident waves walk the same ~1.5 MB of the stream together instead of drifting apart over
    // 118 MB (whole-tree sweep of 1 M reads: 432 ms with one chunk per tile, 235 ms with 80)
    nchunks = std::max<uint32_t>(nchunks, (uint32_t)((sbytes + SWEEP_CHUNK_BYTES - 1) / SWEEP_CHUNK_BYTES));
    nchunks = std::min<uint32_t>(nchunks, (uint32_t)std::max<uint64_t>(1, SWEEP_MAX_PARTIAL_BYTES / ((uint64_t)count * 12)));
    // ... but a chunk's wave pays a set-up (bitmap, read words, checkpoint) worth several blocks: no chunk
    // shorter than 8 blocks, however few tiles the plan has (a plan of a few hundred reads used to be cut into
    // 4096 waves of one or two blocks each)
    nchunks = std::min<uint32_t>(nchunks, std::max<uint32_t>(1, st.NB / 8));
    if (p.dense) nchunks = std::max<uint32_t>(nchunks, DENSE_WAVES_PER_WG);   // one chunk per wave of the workgroup
    nchunks = std::min(nchunks, st.ncp);
    p.bpc = (st.ncp + nchunks - 1) / nchunks * st.cp_stride;
    p.nchunks = (st.NB + p.bpc - 1) / p.bpc;
    if (p.dense) p.nchunks = (p.nchunks + DENSE_WAVES_PER_WG - 1) / DENSE_WAVES_PER_WG * DENSE_WAVES_PER_WG;
}

// info: the routing counters (device_mat.hpp: TI_*) with TI_OFF formed; T: the tile knob; streams / sbytes: the
// handle's m.n_streams streams and the bytes of one sweep of each, wstreams / wbytes its n_wstreams window streams.
inline int plan_launches(const uint32_t* info, uint32_t T, bool walking, bool fuse_windows, const DevMAT& m, const DevStream* streams, const uint64_t* sbytes,
                         const DevStream* wstreams, const uint64_t* wbytes, uint32_t n_wstreams, LaunchPlan& lp) {
    lp = LaunchPlan{};
    lp.arena_maxk = lp.seed_maxk = 1;
    const uint32_t ns = m.n_streams;
    if (m.bm_words * 4 > 128 * 1024) return set_error(WEPP_ELIMIT, "position bitmap does not fit in LDS");
    lp.walk_reads = (uint64_t)info[TI_WCUR] + info[TI_WCUR + 1] + info[TI_RESOLVED] + info[TI_W16WAVE];     // (the plain walk classes: placed by k_route itself or by the blind walks behind it)
    // the window plans share ONE launch (k_sweep_windows): their chunks are sized for the tiles of all of them together
    // (sized per plan, each window asked for enough waves to fill the chip on its own: 1.2 kb reads, 30 windows -- 9
    // workgroups per tile, each rebuilding the tile's table to sweep two blocks of the window's stream)
    uint64_t win_tiles = 0;
    for (uint32_t id = 0; fuse_windows && id < MAX_PLANS; id++) {
        const uint32_t count = info[TI_COUNT + id], maxk = std::max<uint32_t>(1, info[TI_MAXK + id]);
        if (count && plan_class(id) == PLAN_WIN && takes_table(maxk, m.max_pos)) win_tiles += (count + tile_reads(T, maxk) - 1) / tile_reads(T, maxk);
    }
    for (uint32_t id = 0; id < MAX_PLANS; id++) {
        const uint32_t count = info[TI_COUNT + id], maxk = std::max<uint32_t>(1, info[TI_MAXK + id]), off = info[TI_OFF + id];
        if (!count) continue;
        const uint32_t t = plan_index(id), cls = plan_class(id);
        // (slot WC_SLOT of a walk class = the window crowns: one plan, a crown per read; the seeds' plan needs signatures)
        if (cls == PLAN_SEED ? !m.seed_chunks : cls == PLAN_WIN ? t >= n_wstreams : (cls > PLAN_WIN || (t >= ns && !(t == WC_SLOT && m.wc_windows))))
            return set_error(WEPP_EDEVICE, "routing produced an invalid plan id");
        if (cls == PLAN_SEED) {
            // whole-genome samples: a workgroup each, final results written by the kernel (seed_kernels.hip)
            lp.seed_n = count, lp.seed_off = off, lp.seed_maxk = maxk;
        } else if (cls == PLAN_WALKC8 || cls == PLAN_WALKC16) {
            // the reads with many events: their walks are cut into jobs; the plans of a chunked class
            // are the streams, the jobs of stream t numbered behind those of the streams before it
            const uint32_t cc = cls - PLAN_WALKC8;
            lp.walk_reads += count;
            if (walking && !info[TI_JOVER + cc]) continue;     // (launched blind behind k_route)
            WalkPlans& wc = lp.walkc[cc];
            WalkPlanDev& d = wc.p[wc.n];
            d.tier = t;
            d.n_list = info[TI_JOBS + cc * MAX_STREAMS + t];
            d.job0 = (uint32_t)lp.n_jobs[cc];
            d.wave_end = (wc.n ? wc.p[wc.n - 1].wave_end : 0u) + walk_plan_waves(d.n_list);
            wc.n++;
            lp.n_jobs[cc] += d.n_list;
            lp.walkc_reads[cc] += count;
        } else if (cls == PLAN_SWEEP && t == WC_SLOT) {
            // the reads that sweep their window crown, one wave each (k_sweep_arena); one partial per read
            lp.arena_n = count, lp.arena_off = off, lp.arena_maxk = maxk, lp.arena_part = lp.part_total;
            lp.part_total += (size_t)count * 12 * ARENA_CHUNKS;
            if ((uint64_t)count * ARENA_CHUNKS >= (1ull << 31)) return set_error(WEPP_ELIMIT, "too many window-crown sweeps in one call; split the batch");
        } else if (cls != PLAN_WALK8 && cls != PLAN_WALK16) {     // (those two are never counted: k_route places or lists them itself, see walk_reads above)
            TilePlan& p = lp.plans[lp.np++];
            p.window = cls == PLAN_WIN;
            p.t = p.window ? ns - 1 : t;
            p.sid = t;
            p.off = off;
            plan_tiles(p, count, maxk, T, (p.window ? wstreams : streams)[t], (p.window ? wbytes : sbytes)[t], m, fuse_windows ? win_tiles : 0);
            p.part_off = lp.part_total;
            lp.part_total += (size_t)p.nchunks * count * 12;
        }
    }
    if (lp.n_jobs[0] + lp.n_jobs[1] >= (1ull << 31)) return set_error(WEPP_ELIMIT, "too many walk jobs in one call; split the batch");
    if (lp.arena_n && lp.arena_maxk > MAX_TILE_ENTRIES) return set_error(WEPP_ELIMIT, "a read inside one genome window lists more than 8192 positions");
    // The plain (short-read) plans are fused into ONE launch, longest chunks first; the table window plans into another
    // when the handle holds their streams on the device (the workgroups of the largest windows' streams start first);
    // dense and out-of-LDS plans get a launch of their own.  Every tile sweeps its stream once.
    for (uint32_t i = 0; i < lp.np; i++) {
        const TilePlan& p = lp.plans[i];
        if (p.s_in_lds && !p.dense && lp.n_plain < MAX_STREAMS) lp.order[lp.n_plain++] = i;
        else if (p.win_table && fuse_windows && lp.n_wins < MAX_WINDOWS) lp.wins[lp.n_wins++] = i;
        else lp.others[lp.n_other++] = i;
        lp.passes += p.ntiles;
        lp.bytes += (uint64_t)p.ntiles * p.sbytes;
    }
    const auto longer = [&lp](uint32_t a, uint32_t b) { return lp.plans[a].bpc > lp.plans[b].bpc; };
    std::sort(lp.order, lp.order + lp.n_plain, longer);
    std::sort(lp.wins, lp.wins + lp.n_wins, longer);
    // the walks' and the single-launch chains' share of the statistics: a walk "pass" = one wave of 64 reads
    lp.passes += (info[TI_WCUR] + 63) / 64 + (info[TI_WCUR + 1] + 63) / 64 + (info[TI_RESOLVED] + 63) / 64 + info[TI_WWCUR] + info[TI_WWCUR + 1] + (uint64_t)lp.arena_n + lp.seed_n;
    for (uint32_t cc = 0; cc < 2; cc++) {
        if (walking && !info[TI_JOVER + cc]) {
            lp.passes += (info[TI_JCUR + cc] + 63) / 64;
            lp.bytes += (uint64_t)info[TI_CCUR + cc] * 40 + (uint64_t)info[TI_JCUR + cc] * 16;      // (job table, partials, the combination's reads and results)
        }
        if (!lp.walkc[cc].n) continue;
        lp.passes += lp.walkc[cc].p[lp.walkc[cc].n - 1].wave_end;
        // gather (list, count in, count out), scan (in, out), combination (list, offset, count, three partial
        // arrays, four results): what the chain's small kernels move
        lp.bytes += (uint64_t)lp.walkc_reads[cc] * (12 + 8 + 12 + 16) + (uint64_t)(uint32_t)lp.n_jobs[cc] * 12;
    }
    return WEPP_OK;
}

// the `[plan]` line of a tile plan (WEPP_DEBUG_PLANS)
inline void print_plan_line(FILE* to, const TilePlan& p) {
    fprintf(to, "[plan] %s t=%u count=%u off=%u T=%u ntiles=%u nchunks=%u bpc=%u NB=%u ncp=%u dense=%d lds=%u ent_cap=%u key_cap=%u part_off=%zu\n",
            p.window ? "window" : "sweep", p.t, p.count, p.off, p.T, p.ntiles, p.nchunks, p.bpc, p.NB, p.ncp, (int)p.dense,
            p.lds_bytes, p.ent_cap, p.key_cap, p.part_off);
}

}  // namespace wepp
