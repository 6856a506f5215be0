// epp_sweep.cpp -- the planning and launch part of wepp_epp_map as routines (declared in epp_host.hpp): the sweep of
// a list of reads in two passes, and the map's body on top of it.  wepp_epp_map (epp_capi.cpp) runs the body over a
// batch; wepp_epp_peaks (peaks_capi.cpp) runs it once, keeps what it leaves on the device and sweeps every subset of
// reads it removes once more into the same difference array.
//
// The reference walks, for every read, a range tree (arena.cpp:68-169) recursively and
// updates the haplotypes' scores under a mutex.  Here the reads are sorted by window,
// cut into tiles of 64 and groups of tiles; every group gets the slice of the MAT's EPP
// event stream that falls into its genome window, and two sweeps of (tile, chunk) jobs
// produce the per-read and per-haplotype results (epp_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "epp.hpp"
#include "epp_host.hpp"
#include "staged_copy.hpp"

namespace wepp {

namespace {

// jobs (tile, stream chunk) a call aims at (WEPP_EPP_TARGET_JOBS): see wepp_epp_map
constexpr uint32_t EPP_TARGET_JOBS = 262144;   // measured at 16 M nodes, 1 M reads: 8192 (one chunk per tile, 15.6 K jobs) 576 ms, 32 K 440, 64 K 402, 128 K 382, 256 K 370, 1 M 362, 4 M 379 ms on the device

}  // namespace

int epp_sweep_pass1(wepp_mat_t* mat, DevPool& pool, const wepp_epp_reads* rd, const std::vector<uint32_t>& order, const DevReads& reads,
                    uint32_t genome_size, double fx_scale, hipStream_t stream, hipEvent_t begin, hipEvent_t selected, EppSweep* sw) {
    const uint32_t R = (uint32_t)order.size();
    const uint32_t N = mat->dev.N;
    // ---- tiles, groups ----------------------------------------------------------------------
    // reads per lane.  4 shares the serial per-event work (broadcasts, flips, atomics) among 256 reads
    // per wave, but a tile that large lists almost every position of its window, so every event takes
    // the allele-lookup path: measured 1.4x slower than 1 -- kept selectable for
    // experiments, and only while its allele table leaves room for several waves per CU.
    uint32_t rpl = 1;
    if (const char* env = std::getenv("WEPP_EPP_RPL")) rpl = std::atoi(env) == 4 ? 4 : 1;
    if (rpl == 4) {
        int32_t longest = 0;
        for (uint32_t s = 0; s < R; s++) longest = std::max(longest, rd->end[order[s]] - rd->start[order[s]]);
        if ((((uint32_t)longest >> 3) + 1) * 64 * 4 * 4 > 48 * 1024) rpl = 1;
    }
    const uint32_t TS = 64 * rpl;
    const uint32_t ntiles = (R + TS - 1) / TS;
    const uint32_t tpg = std::max<uint32_t>(1, (ntiles + EPP_MAX_GROUPS - 1) / EPP_MAX_GROUPS);
    const uint32_t G = (ntiles + tpg - 1) / tpg;
    std::vector<EppGroup> groups(G);
    std::vector<uint32_t> we_max(G);
    uint32_t bm_words = 1, max_span = 0;
    for (uint32_t g = 0; g < G; g++) {
        EppGroup& gr = groups[g];
        gr = EppGroup{};
        gr.tile0 = g * tpg;
        gr.ntiles = std::min(tpg, ntiles - gr.tile0);
        gr.ws = 0xFFFFFFFFu;
        gr.we = 0;
        for (uint32_t t = gr.tile0; t < gr.tile0 + gr.ntiles; t++) {
            uint32_t ts = 0xFFFFFFFFu, te = 0;
            for (uint32_t s = t * TS; s < std::min<uint64_t>(R, (uint64_t)t * TS + TS); s++) {
                const uint32_t r = order[s];
                ts = std::min(ts, (uint32_t)rd->start[r]);
                te = std::max(te, (uint32_t)rd->end[r]);
                max_span = std::max(max_span, (uint32_t)(rd->end[r] - rd->start[r]));
            }
            bm_words = std::max(bm_words, ((te - ts) >> 5) + 1);
            gr.ws = std::min(gr.ws, ts);
            gr.we = std::max(gr.we, te);
        }
        we_max[g] = g ? std::max(we_max[g - 1], gr.we) : gr.we;
    }
    // per-read allele table: one nibble per window position, 8 positions per word, lane-interleaved
    const uint32_t tab_rows = (max_span >> 3) + 1;
    const uint32_t lds_bytes = (bm_words + tab_rows * 64 * rpl) * 4;
    if (lds_bytes > 150 * 1024)
        return set_error(WEPP_ELIMIT, "a tile of 64 reads needs " + std::to_string(lds_bytes) +
                                          " bytes of LDS (window bitmap + allele table): reads too long");

    uint32_t* d_wemax;
    EppGroup* d_groups;
    DEV_GET(pool, d_groups, G); DEV_GET(pool, d_wemax, G);
    HIP_TRY(hipMemcpyAsync(d_groups, groups.data(), (size_t)G * sizeof(EppGroup), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_wemax, we_max.data(), (size_t)G * 4, hipMemcpyHostToDevice, stream));
    if (begin) HIP_TRY(hipEventRecord(begin, stream));

    // ---- window streams --------------------------------------------------------------------
    const uint64_t E = mat->epp_events;
    const uint32_t nblk = (uint32_t)((E + EPP_SEL_EVENTS - 1) / EPP_SEL_EVENTS);
    uint32_t *d_cnt, *d_totals;
    DEV_GET(pool, d_cnt, (size_t)G * std::max<uint32_t>(nblk, 1)); DEV_GET(pool, d_totals, G);
    std::vector<uint32_t> totals(G, 0);
    if (nblk) {
        HIP_TRY(launch_epp_select_count(mat->epp_word, E, d_groups, d_wemax, G, nblk, d_cnt, stream));
        HIP_TRY(launch_epp_select_scan(d_cnt, G, nblk, d_totals, stream));
        HIP_TRY(hipMemcpyAsync(totals.data(), d_totals, (size_t)G * 4, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    uint64_t total_events = 0, swept = 0;
    uint32_t n_max = 0;
    for (uint32_t g = 0; g < G; g++) {
        groups[g].n_events = totals[g];
        groups[g].soff = total_events;
        total_events += totals[g];
        n_max = std::max(n_max, totals[g]);
        swept += (uint64_t)totals[g] * groups[g].ntiles;
    }
    // enough jobs to fill the machine when there are few tiles
    static const uint32_t target_jobs = getenv("WEPP_EPP_TARGET_JOBS") ? (uint32_t)std::max(1, atoi(getenv("WEPP_EPP_TARGET_JOBS"))) : EPP_TARGET_JOBS;
    const uint32_t want_chunks = std::max<uint32_t>(1, (target_jobs + ntiles - 1) / ntiles);
    uint32_t chunk_events = std::max<uint32_t>(1024, (n_max + want_chunks - 1) / want_chunks);
    chunk_events = (chunk_events + 63) & ~63u;
    uint64_t n_jobs64 = 0;
    for (uint32_t g = 0; g < G; g++) {
        groups[g].nchunks = std::max<uint32_t>(1, (groups[g].n_events + chunk_events - 1) / chunk_events);
        groups[g].job0 = (uint32_t)n_jobs64;
        n_jobs64 += (uint64_t)groups[g].nchunks * groups[g].ntiles;
    }
    if (n_jobs64 >= (1ull << 31)) return set_error(WEPP_ELIMIT, "too many sweep jobs");
    const uint32_t n_jobs = (uint32_t)n_jobs64;
    HIP_TRY(hipMemcpyAsync(d_groups, groups.data(), (size_t)G * sizeof(EppGroup), hipMemcpyHostToDevice, stream));
    uint32_t *d_stw, *d_stn;
    DEV_GET(pool, d_stw, total_events); DEV_GET(pool, d_stn, total_events);
    if (nblk) HIP_TRY(launch_epp_select_scatter(mat->epp_word, mat->epp_node, E, d_groups, d_wemax, G, nblk, d_cnt, d_stw, d_stn, stream));
    if (selected) HIP_TRY(hipEventRecord(selected, stream));

    // ---- pass 1, combine -------------------------------------------------------------------
    const size_t rows = (size_t)n_jobs * 64 * rpl;
    int32_t *d_pmin, *d_pnet, *d_best;
    uint32_t *d_pcnt, *d_mult;
    long long* d_fx;
    DEV_GET(pool, d_pmin, rows); DEV_GET(pool, d_pcnt, rows); DEV_GET(pool, d_pnet, rows); DEV_GET(pool, d_best, R); DEV_GET(pool, d_mult, R); DEV_GET(pool, d_fx, R);
    EppSweepArgs a{};
    a.groups = d_groups; a.G = G; a.n_jobs = n_jobs; a.R = R; a.N = N;
    a.chunk_events = chunk_events; a.bm_words = bm_words; a.tab_rows = tab_rows;
    a.bin_size = genome_size / EPP_BINS;
    a.st_word = d_stw; a.st_node = d_stn;
    a.read_off = reads.read_off; a.read_word = reads.read_word; a.start = reads.start; a.end = reads.end; a.degree = reads.degree; a.order = reads.order;
    a.part_min = d_pmin; a.part_cnt = d_pcnt; a.part_net = d_pnet;
    a.best = d_best; a.mult = d_mult; a.delta_fx = d_fx;
    a.fx_scale = fx_scale;
    HIP_TRY(launch_epp_sweep(a, 1, rpl, lds_bytes, stream));
    HIP_TRY(launch_epp_combine(a, tpg, rpl, stream));
    sw->a = a;
    sw->rpl = rpl; sw->lds_bytes = lds_bytes; sw->tiles_per_group = tpg;
    sw->events_swept = swept; sw->stream_events = total_events;
    return WEPP_OK;
}

int epp_sweep_pass2(const EppSweep& sw, const long long* delta_fx, const uint64_t* epp_base, uint32_t* epp_nodes,
                    unsigned long long* diff_score, int* diff_cnt, hipStream_t stream) {
    EppSweepArgs a = sw.a;
    if (delta_fx) a.delta_fx = const_cast<long long*>(delta_fx);
    a.epp_base = epp_base; a.epp_nodes = epp_nodes; a.diff_score = diff_score; a.diff_cnt = diff_cnt;
    HIP_TRY(launch_epp_sweep(a, 2, sw.rpl, sw.lds_bytes, stream));
    return WEPP_OK;
}

int epp_map_run(wepp_mat_t* mat, DevPool& pool, const wepp_epp_reads* rd, uint32_t genome_size, uint32_t max_cached_epp,
                long long total_degree, wepp_epp_out* out, bool want_divergence, EppMapState* st) {
    const uint32_t R = rd->n_reads;
    const uint32_t N = mat->dev.N;
    hipStream_t stream = nullptr;

    // ---- reads in window order, on the device ----------------------------------------------
    std::vector<uint32_t>& order = st->order;
    epp_window_order(rd, order);
    DevReads& reads = st->reads;
    if (int rc = upload_reads(pool, rd, order, stream, &reads)) return rc;

    DevEvents<5> ev;
    if (int rc = ev.create()) return rc;

    int fx_bits = 62;
    for (long long s = total_degree; s > 0; s >>= 1) fx_bits--;
    fx_bits = std::min(fx_bits, 52);
    st->fx_scale = std::ldexp(1.0, fx_bits);
    EppSweep& sw = st->sweep;
    if (int rc = epp_sweep_pass1(mat, pool, rd, order, reads, genome_size, st->fx_scale, stream, ev[0], ev[1], &sw)) return rc;
    const EppSweepArgs& a = sw.a;
    std::vector<int32_t> best_s(R);
    std::vector<uint32_t> mult_s(R);
    HIP_TRY(hipMemcpyAsync(best_s.data(), a.best, (size_t)R * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(mult_s.data(), a.mult, (size_t)R * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(ev[2], stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (uint32_t s = 0; s < R; s++) {
        out->max_parsimony[order[s]] = best_s[s];
        out->multiplicity[order[s]] = mult_s[s];
    }
    // EPP lists of the reads with few enough placements (initial_filter.cpp:205-210)
    std::vector<uint64_t> epp_base(R, ~0ull);
    uint64_t epp_total = 0;
    bool lists_overflow = false;
    if (out->epp_off) {
        out->epp_off[0] = 0;
        for (uint32_t r = 0; r < R; r++) {
            if (out->multiplicity[r] <= max_cached_epp) { epp_base[r] = epp_total; epp_total += out->multiplicity[r]; }
            out->epp_off[r + 1] = epp_total;
        }
        // too small a list buffer does not stop the call: everything else is computed and delivered, the lists stay
        // with the handle for wepp_epp_fetch_lists, and the call reports WEPP_ELIMIT at its end
        lists_overflow = epp_total > out->epp_capacity || (epp_total && !out->epp_nodes);
    }
    mat->epp_pending.clear();

    // ---- pass 2 ----------------------------------------------------------------------------
    const bool want_cnt = out->hap_read_counts || out->hap_divergence || want_divergence;
    uint64_t* d_ebase;
    uint32_t* d_enodes;
    unsigned long long* d_dscore;
    int* d_dcnt = nullptr;
    DEV_GET(pool, d_ebase, R); DEV_GET(pool, d_enodes, epp_total); DEV_GET(pool, d_dscore, (size_t)N + 1);
    if (want_cnt) DEV_GET(pool, d_dcnt, ((size_t)N + 1) * EPP_BINS);
    HIP_TRY(hipMemcpyAsync(d_ebase, epp_base.data(), (size_t)R * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_dscore, 0, ((size_t)N + 1) * 8, stream));
    if (want_cnt) HIP_TRY(hipMemsetAsync(d_dcnt, 0, ((size_t)N + 1) * EPP_BINS * 4, stream));
    if (int rc = epp_sweep_pass2(sw, nullptr, d_ebase, d_enodes, d_dscore, d_dcnt, stream)) return rc;
    HIP_TRY(hipEventRecord(ev[3], stream));

    // ---- prefix sums -> per-haplotype outputs ------------------------------------------------
    double *d_score, *d_div = nullptr;
    int *d_counts = nullptr, *d_true = nullptr;
    void* d_scratch;
    DEV_GET(pool, d_score, N);
    {
        char* sc;
        DEV_GET(pool, sc, epp_finish_scratch_bytes(N));
        d_scratch = sc;
    }
    int true_counts[EPP_BINS] = {0};
    if (want_cnt) {
        // arena::build_range_trees, arena.cpp:137-147
        for (uint32_t r = 0; r < R; r++)
            true_counts[std::min<uint32_t>((uint32_t)rd->start[r] / a.bin_size, EPP_BINS - 1)] += rd->degree[r];
        DEV_GET(pool, d_true, EPP_BINS);
        HIP_TRY(hipMemcpyAsync(d_true, true_counts, sizeof(true_counts), hipMemcpyHostToDevice, stream));
        if (out->hap_read_counts) DEV_GET(pool, d_counts, (size_t)N * EPP_BINS);
        if (out->hap_divergence || want_divergence) DEV_GET(pool, d_div, N);
    }
    HIP_TRY(launch_epp_finish(N, d_dscore, 1.0 / a.fx_scale, d_score, d_dcnt, d_true, d_counts, d_div, d_scratch, stream));
    HIP_TRY(hipEventRecord(ev[4], stream));
    // the per-haplotype outputs are gigabytes at 16 M nodes: staged copies (staged_copy.hpp)
    HIP_TRY(d2h_staged(out->hap_score, d_score, (size_t)N * 8, stream));
    if (d_counts) HIP_TRY(d2h_staged(out->hap_read_counts, d_counts, (size_t)N * EPP_BINS * 4, stream));
    if (d_div && out->hap_divergence) HIP_TRY(d2h_staged(out->hap_divergence, d_div, (size_t)N * 8, stream));
    if (epp_total && lists_overflow) {
        try { mat->epp_pending.resize(epp_total); } catch (const std::bad_alloc&) {
            return set_error(WEPP_ENOMEM, "out of host memory for " + std::to_string(epp_total) + " EPP list entries");
        }
        HIP_TRY(d2h_staged(mat->epp_pending.data(), d_enodes, epp_total * 4, stream));
    } else if (epp_total) HIP_TRY(d2h_staged(out->epp_nodes, d_enodes, epp_total * 4, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    (void)hipEventElapsedTime(&st->select_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&st->sweep1_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&st->sweep2_ms, ev[2], ev[3]);
    (void)hipEventElapsedTime(&st->finish_ms, ev[3], ev[4]);
    st->groups = a.G;
    st->jobs = a.n_jobs;
    st->diff_score = d_dscore; st->score = d_score; st->divergence = d_div; st->scan_scratch = d_scratch;
    if (lists_overflow)
        return set_error(WEPP_ELIMIT, "epp_nodes holds " + std::to_string(out->epp_capacity) + " entries, " + std::to_string(epp_total) +
                                      " needed: every other output is complete, fetch the lists with wepp_epp_fetch_lists");
    return WEPP_OK;
}

}  // namespace wepp
