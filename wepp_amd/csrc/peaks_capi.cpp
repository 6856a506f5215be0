// peaks_capi.cpp -- wepp_epp_peaks: host side of the peak-removal loop of wepp_filter
// (`while (!step(...))`, src/WEPP/initial_filter.cpp:241-453, behind cartesian_map).
//
// The reference keeps the EPP lists of the reads with few placements and recomputes the others' distances; both
// compute the same thing, which is all that runs here.  The map runs first and leaves the fixed-point difference
// array of the scores, P (max_parsimony), M and q (the integer every EPP haplotype of a read received) on the device.
// A step then is: prefix sums -> scores -> leader and tie group (k_peak_max / k_peak_ties); the walk over the group
// on the host (peak_select.hpp) with the distances out of one distance field per accepted peak (the kernels of
// wepp_epp_neighbors, whose second scan also yields the region that becomes `mapped`); k_peak_hits for the reads the
// accepted peaks correspond to; and the map's own two passes over those reads with -q, into the same array.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../host/peak_select.hpp"
#include "epp_host.hpp"
#include "neighbors.hpp"
#include "peaks.hpp"
#include "staged_copy.hpp"

namespace {

struct PeaksTiming { double map_ms = 0, select_ms = 0, hits_ms = 0, remove_ms = 0, clear_ms = 0; };
thread_local PeaksTiming g_last;

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

void zero_outputs(const wepp_peaks_out* out, uint32_t R, uint32_t N, uint32_t max_peaks) {
    *out->n_peaks = 0; *out->n_steps = 0; *out->n_remaining = R;
    std::fill(out->peaks, out->peaks + max_peaks, 0xFFFFFFFFu);
    std::fill(out->peak_step, out->peak_step + max_peaks, 0u);
    std::fill(out->peak_reads, out->peak_reads + max_peaks, 0u);
    std::fill(out->peak_degree, out->peak_degree + max_peaks, (int64_t)0);
    std::fill(out->peak_score, out->peak_score + max_peaks, 0.0);
    if (R) { std::fill(out->removed_step, out->removed_step + R, -1); std::fill(out->removed_peak, out->removed_peak + R, 0xFFFFFFFFu); }
    std::fill(out->mapped, out->mapped + N, (uint8_t)0);
    if (out->score_left) std::fill(out->score_left, out->score_left + N, 0.0);
}

// The device blocks of the field passes, taken once per call: one pivot per pass, in a table of NBR_LANE_COLS columns
struct FieldBlocks {
    uint32_t Es = NBR_LANE_COLS, nblk = 0;
    int32_t *field = nullptr, *over = nullptr, *tover = nullptr, *gdist = nullptr;
    uint32_t *piv = nullptr, *bsum = nullptr, *bcnt = nullptr, *top = nullptr, *tend = nullptr, *nreg = nullptr, *nlist = nullptr;
    unsigned long long* off = nullptr;
    char* temp = nullptr;
    size_t temp_bytes = 0;
};

int alloc_field_blocks(DevPool& pool, uint32_t N, FieldBlocks* f) {
    const uint64_t rows = (uint64_t)N + 1;
    const uint32_t Es = f->Es;
    f->nblk = nbr_scan_blocks((uint32_t)rows);
    DEV_GET(pool, f->piv, 1); DEV_GET(pool, f->field, rows * Es); DEV_GET(pool, f->over, rows * Es); DEV_GET(pool, f->gdist, N);
    DEV_GET(pool, f->bsum, (size_t)f->nblk * Es); DEV_GET(pool, f->bcnt, (size_t)f->nblk * Es);
    DEV_GET(pool, f->top, Es); DEV_GET(pool, f->tend, Es); DEV_GET(pool, f->tover, Es); DEV_GET(pool, f->nreg, Es);
    DEV_GET(pool, f->nlist, (size_t)Es + 1); DEV_GET(pool, f->off, (size_t)Es + 1);
    HIP_TRY(assign_scan_temp_bytes(Es, &f->temp_bytes));
    DEV_GET(pool, f->temp, f->temp_bytes);
    return WEPP_OK;
}

// One accepted peak: its distances to the n_group haplotypes of d_group (-> dist), and its WEPP_NBR_FROM_PIVOT region of
// `radius` -> mapped.  select_ms / clear_ms receive the wall time of the two halves.
int field_pass(wepp_mat_t* mat, const FieldBlocks& f, uint32_t pivot, uint32_t radius, const uint32_t* d_group, uint32_t n_group,
               std::vector<int32_t>& dist, uint8_t* d_mapped, hipStream_t stream, hipEvent_t e0, hipEvent_t e1, PeaksTiming* tm) {
    const uint32_t N = mat->dev.N, Es = f.Es;
    const uint64_t rows = (uint64_t)N + 1;
    Clock::time_point t0 = Clock::now();
    DevPool pass_pool(mat->epp_cache);          // the pass's genotype table and region list: back in the cache for the next pass
    AssignTable tab;
    if (int rc = assign_build_table(mat, pass_pool, 1, &pivot, stream, e0, e1, &tab)) return rc;
    NbrTree t{};
    t.N = N; t.max_pos = mat->dev.max_pos;
    t.node_woff = mat->dev.node_woff; t.words = mat->dev.words; t.parent_dfs = mat->dev.parent_dfs; t.dfs_end = mat->nbr_dfs_end;
    HIP_TRY(hipMemcpyAsync(f.piv, &pivot, 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(f.field, 0, rows * Es * 4, stream));
    HIP_TRY(launch_nbr_deltas(t, tab.geno, tab.Kp, Es, WEPP_NBR_FROM_PIVOT, f.field, stream));
    HIP_TRY(launch_nbr_colscan(f.field, Es, N, f.bsum, stream));
    dist.resize(n_group);
    HIP_TRY(launch_peak_gather(f.field, Es, 0, N, d_group, n_group, f.gdist, stream));
    if (n_group) HIP_TRY(hipMemcpyAsync(dist.data(), f.gdist, (size_t)n_group * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    tm->select_ms += ms_since(t0);
    // ---- the region --------------------------------------------------------------------------------------
    t0 = Clock::now();
    HIP_TRY(hipMemsetAsync(f.over, 0, rows * Es * 4, stream));
    HIP_TRY(hipMemsetAsync(f.nreg, 0, (size_t)Es * 4, stream));
    HIP_TRY(hipMemsetAsync(f.nlist, 0, ((size_t)Es + 1) * 4, stream));
    HIP_TRY(launch_nbr_over(t, f.field, Es, radius, f.over, stream));
    HIP_TRY(launch_nbr_colscan(f.over, Es, N, f.bsum, stream));
    HIP_TRY(launch_nbr_tops(t, f.piv, 1, f.field, f.over, Es, radius, f.top, f.tend, f.tover, stream));
    HIP_TRY(launch_nbr_count(N, f.over, Es, f.top, f.tend, f.tover, nullptr, f.bcnt, f.nreg, f.nlist, stream));
    HIP_TRY(launch_assign_scan(f.nlist, f.off, 1, f.temp, f.temp_bytes, stream));
    unsigned long long off[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(off, f.off, sizeof(off), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t need = off[1];
    if (need > N) return set_error(WEPP_EDEVICE, "a region of " + std::to_string(need) + " haplotypes on a tree of " + std::to_string(N));
    if (need) {
        uint32_t* d_node;
        int32_t* d_dist;
        DEV_GET(pass_pool, d_node, need); DEV_GET(pass_pool, d_dist, need);
        HIP_TRY(launch_nbr_write(N, 1, f.field, f.over, Es, f.top, f.tend, f.tover, nullptr, f.bcnt, f.off, d_node, d_dist, stream));
        HIP_TRY(launch_peak_mark(d_node, need, N, d_mapped, stream));
    }
    HIP_TRY(launch_peak_mark(f.piv, 1, N, d_mapped, stream));      // (the peak itself, whatever its region)
    HIP_TRY(hipStreamSynchronize(stream));
    tm->clear_ms += ms_since(t0);
    return WEPP_OK;
}

}  // namespace

extern "C" int wepp_epp_peaks_last_timing(double* map_ms, double* select_ms, double* hits_ms, double* remove_ms, double* clear_ms) {
    if (map_ms) *map_ms = g_last.map_ms;
    if (select_ms) *select_ms = g_last.select_ms;
    if (hits_ms) *hits_ms = g_last.hits_ms;
    if (remove_ms) *remove_ms = g_last.remove_ms;
    if (clear_ms) *clear_ms = g_last.clear_ms;
    return WEPP_OK;
}

extern "C" int wepp_epp_peaks(wepp_mat_t* mat, const wepp_epp_reads* rd, uint32_t genome_size, const wepp_peaks_params* par,
                              const uint32_t* tie_rank, wepp_epp_out* map_out, wepp_peaks_out* out) {
    if (!mat || !rd || !par || !out) return set_error(WEPP_EINVAL, "null argument");
    if (par->top_n == 0 || par->max_peaks == 0) return set_error(WEPP_EINVAL, "top_n and max_peaks must be at least 1");
    const uint32_t R = rd->n_reads;
    const uint32_t N = mat->dev.N;
    if (R && (!rd->read_off || !rd->start || !rd->end || !rd->degree)) return set_error(WEPP_EINVAL, "null read array");
    if (!out->n_peaks || !out->n_steps || !out->n_remaining || !out->peaks || !out->peak_step || !out->peak_reads || !out->peak_degree ||
        !out->peak_score || !out->mapped || (R && (!out->removed_step || !out->removed_peak)))
        return set_error(WEPP_EINVAL, "null output array");
    if (map_out) {
        if (!map_out->max_parsimony || !map_out->multiplicity || !map_out->hap_score) return set_error(WEPP_EINVAL, "null output array");
        if ((map_out->epp_off == nullptr) != (map_out->epp_nodes == nullptr)) return set_error(WEPP_EINVAL, "epp_off and epp_nodes go together");
    }
    if (genome_size < EPP_BINS) return set_error(WEPP_EINVAL, "genome_size must be at least NUM_RANGE_BINS (50)");
    const uint64_t W = R ? rd->read_off[R] : 0;
    if (W && !rd->read_word) return set_error(WEPP_EINVAL, "null read_word");
    if (W >= (1ull << 32)) return set_error(WEPP_ELIMIT, "more than 2^32 read words in one call");
    long long total_degree = 0;
    if (int rc = epp_validate_reads(rd, &total_degree)) return rc;
    const PeakLimits lim{par->top_n, par->max_peaks, par->peak_radius};
    const double eps = par->score_epsilon;
    g_last = PeaksTiming{};
    zero_outputs(out, R, N, lim.max_peaks);
    if (R == 0) {
        if (map_out) {
            std::fill(map_out->hap_score, map_out->hap_score + N, 0.0);
            if (map_out->hap_read_counts) std::fill(map_out->hap_read_counts, map_out->hap_read_counts + (size_t)N * EPP_BINS, 0);
            if (map_out->hap_divergence) std::fill(map_out->hap_divergence, map_out->hap_divergence + N, std::nan(""));
            if (map_out->epp_off) map_out->epp_off[0] = 0;
        }
        return WEPP_OK;
    }
    HIP_TRY(hipSetDevice(mat->device));
    if (int rc = nbr_prepare_handle(mat)) return rc;
    hipStream_t stream = nullptr;

    // ---- the map: scores, P, M, q and the difference array stay on the device ----------------------------------
    Clock::time_point t0 = Clock::now();
    DevPool pool(mat->epp_cache);
    EppMapState st;
    std::vector<int32_t> own_p;
    std::vector<uint32_t> own_m;
    std::vector<double> own_score;
    wepp_epp_out mo{};
    if (map_out) mo = *map_out;
    else {
        own_p.resize(R); own_m.resize(R); own_score.resize(N);
        mo.max_parsimony = own_p.data(); mo.multiplicity = own_m.data(); mo.hap_score = own_score.data();
    }
    if (int rc = epp_map_run(mat, pool, rd, genome_size, WEPP_MAX_CACHED_EPP_SIZE, total_degree, &mo, true, &st)) return rc;
    g_last.map_ms = ms_since(t0);
    const std::vector<uint32_t>& order = st.order;

    // ---- the loop's own state ----------------------------------------------------------------------------------
    uint8_t *d_mapped, *d_alive;
    PeakTop* d_top;
    uint32_t *d_group, *d_hits, *d_nhits, *d_preads, *d_rpeak;
    double* d_gfull;
    int32_t* d_rstep;
    unsigned long long* d_pdeg;
    uint64_t* d_nolist;
    DEV_GET(pool, d_mapped, N); DEV_GET(pool, d_alive, R); DEV_GET(pool, d_top, 1); DEV_GET(pool, d_group, N); DEV_GET(pool, d_gfull, N);
    DEV_GET(pool, d_hits, R); DEV_GET(pool, d_nhits, 1); DEV_GET(pool, d_preads, lim.max_peaks); DEV_GET(pool, d_pdeg, lim.max_peaks);
    DEV_GET(pool, d_rstep, R); DEV_GET(pool, d_rpeak, R); DEV_GET(pool, d_nolist, R);
    FieldBlocks fb;
    if (int rc = alloc_field_blocks(pool, N, &fb)) return rc;
    HIP_TRY(hipMemsetAsync(d_mapped, 0, N, stream));
    HIP_TRY(hipMemsetAsync(d_alive, 1, R, stream));
    HIP_TRY(hipMemsetAsync(d_preads, 0, (size_t)lim.max_peaks * 4, stream));
    HIP_TRY(hipMemsetAsync(d_pdeg, 0, (size_t)lim.max_peaks * 8, stream));
    HIP_TRY(hipMemsetAsync(d_rstep, 0xFF, (size_t)R * 4, stream));
    HIP_TRY(hipMemsetAsync(d_rpeak, 0xFF, (size_t)R * 4, stream));
    HIP_TRY(hipMemsetAsync(d_nolist, 0xFF, (size_t)R * 8, stream));      // (~0: no read of a removal keeps a list)
    DevEvents<2> ev;
    if (int rc = ev.create()) return rc;

    const double inv_scale = 1.0 / st.fx_scale;
    uint32_t n_peaks = 0, n_steps = 0, n_remaining = R;
    bool scores_current = true;            // st.score holds the prefix sums of the difference array as it is
    std::vector<uint32_t> group, hits, sub_order;
    std::vector<double> gfull;
    std::vector<std::vector<int32_t>> dist;           // per accepted peak of the step: its distances to the tie group

    while (true) {
        // ---- leader and tie group ---------------------------------------------------------------------------
        t0 = Clock::now();
        if (!scores_current) {
            HIP_TRY(launch_epp_finish(N, st.diff_score, inv_scale, st.score, nullptr, nullptr, nullptr, nullptr, st.scan_scratch, stream));
            scores_current = true;
        }
        if (peak_done(n_peaks, lim.max_peaks, n_remaining)) break;
        HIP_TRY(hipMemsetAsync(d_top, 0, sizeof(PeakTop), stream));
        HIP_TRY(launch_peak_max(N, st.score, st.divergence, d_mapped, eps, d_top, stream));
        HIP_TRY(launch_peak_ties(N, st.score, st.divergence, d_mapped, eps, d_top, d_group, d_gfull, stream));
        PeakTop top{};
        HIP_TRY(hipMemcpyAsync(&top, d_top, sizeof(top), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        double m;
        std::memcpy(&m, &top.m_bits, 8);
        if (peak_no_leader(top.n_live, m, eps)) { g_last.select_ms += ms_since(t0); break; }
        const uint32_t n_group = std::min(top.n_tie, N);
        group.resize(n_group); gfull.resize(n_group);
        HIP_TRY(hipMemcpyAsync(group.data(), d_group, (size_t)n_group * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(gfull.data(), d_gfull, (size_t)n_group * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        peak_order_group(group, tie_rank, &gfull);
        // the field passes gather by place in the ORDERED group
        HIP_TRY(hipMemcpyAsync(d_group, group.data(), (size_t)n_group * 4, hipMemcpyHostToDevice, stream));
        g_last.select_ms += ms_since(t0);

        // ---- consideration: one field pass per accepted peak, made when the walk first asks for its distances ------
        dist.clear();
        std::vector<uint32_t> acc_nodes, pass_place;        // pass_place[k]: the place in the group of the peak of pass k
        int pass_rc = WEPP_OK;
        auto pass_of = [&](uint32_t place) -> size_t {
            size_t k = std::find(pass_place.begin(), pass_place.end(), place) - pass_place.begin();
            if (k == pass_place.size() && pass_rc == WEPP_OK) {
                pass_place.push_back(place);
                dist.emplace_back();
                pass_rc = field_pass(mat, fb, group[place], lim.peak_radius, d_group, n_group, dist.back(), d_mapped, stream, ev[0], ev[1], &g_last);
            }
            return k;
        };
        const std::vector<uint32_t> accepted_places = peak_consider(n_group, n_peaks, lim, [&](uint32_t old, uint32_t cand) -> long long {
            const size_t k = pass_of(old);
            return pass_rc == WEPP_OK ? dist[k][cand] : 0;      // (a failed pass rejects the rest; the call fails below)
        });
        if (pass_rc != WEPP_OK) return pass_rc;
        for (uint32_t place : accepted_places) {
            (void)pass_of(place);                               // (the last accepted: nobody asked for its distances)
            if (pass_rc != WEPP_OK) return pass_rc;
            acc_nodes.push_back(group[place]);
        }
        const uint32_t K = (uint32_t)acc_nodes.size();
        if (K == 0) break;                                  // (cannot happen: the first candidate has nobody to object)
        for (uint32_t k = 0; k < K; k++) {
            out->peaks[n_peaks + k] = acc_nodes[k];
            out->peak_step[n_peaks + k] = n_steps;
            out->peak_score[n_peaks + k] = gfull[accepted_places[k]];
        }

        // ---- the reads of the accepted peaks ---------------------------------------------------------------------
        t0 = Clock::now();
        uint32_t n_hits = 0;
        {
            DevPool step_pool(mat->epp_cache);
            AssignTable tab;
            if (int rc = assign_build_table(mat, step_pool, K, acc_nodes.data(), stream, ev[0], ev[1], &tab)) return rc;
            HIP_TRY(hipMemsetAsync(d_nhits, 0, 4, stream));
            PeakHitsArgs h{};
            h.R = R; h.K = K; h.Kp = tab.Kp; h.max_pos = tab.max_pos; h.geno = tab.geno; h.pre = tab.pre;
            h.read_off = st.reads.read_off; h.read_word = st.reads.read_word; h.start = st.reads.start; h.end = st.reads.end;
            h.degree = st.reads.degree; h.order = st.reads.order;
            h.best = st.sweep.a.best; h.alive = d_alive; h.step = (int32_t)n_steps; h.peak_base = n_peaks;
            h.removed_step = d_rstep; h.removed_peak = d_rpeak; h.hits = d_hits; h.n_hits = d_nhits;
            h.peak_reads = d_preads; h.peak_degree = d_pdeg;
            HIP_TRY(launch_peak_hits(h, stream));
            HIP_TRY(hipMemcpyAsync(&n_hits, d_nhits, 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (n_hits > n_remaining) return set_error(WEPP_EDEVICE, "more reads removed than remained");
            hits.resize(n_hits);
            if (n_hits) HIP_TRY(hipMemcpyAsync(hits.data(), d_hits, (size_t)n_hits * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        g_last.hits_ms += ms_since(t0);

        // ---- removal: the subset through the map's sweep, -q into the same difference array ----------------------
        t0 = Clock::now();
        if (n_hits) {
            std::sort(hits.begin(), hits.end());            // places ascending = window order
            sub_order.resize(n_hits);
            for (uint32_t i = 0; i < n_hits; i++) {
                if (hits[i] >= R) return set_error(WEPP_EDEVICE, "a removed read's place is out of range");
                sub_order[i] = order[hits[i]];
            }
            DevPool step_pool(mat->epp_cache);
            uint32_t *d_places, *d_suborder;
            DEV_GET(step_pool, d_places, n_hits); DEV_GET(step_pool, d_suborder, n_hits);
            HIP_TRY(hipMemcpyAsync(d_places, hits.data(), (size_t)n_hits * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_suborder, sub_order.data(), (size_t)n_hits * 4, hipMemcpyHostToDevice, stream));
            DevReads sub = st.reads;
            sub.order = d_suborder;
            EppSweep sw;
            if (int rc = epp_sweep_pass1(mat, step_pool, rd, sub_order, sub, genome_size, st.fx_scale, stream, nullptr, nullptr, &sw)) return rc;
            // the shares the map handed out, not what the subset's own combine would give them
            HIP_TRY(launch_peak_negq(n_hits, d_places, st.sweep.a.delta_fx, sw.a.delta_fx, stream));
            if (int rc = epp_sweep_pass2(sw, nullptr, d_nolist, nullptr, st.diff_score, nullptr, stream)) return rc;
            HIP_TRY(hipStreamSynchronize(stream));
            scores_current = false;
        }
        g_last.remove_ms += ms_since(t0);
        n_remaining -= n_hits;
        n_peaks += K;
        n_steps++;
    }

    // ---- outputs ---------------------------------------------------------------------------------------------------
    *out->n_peaks = n_peaks; *out->n_steps = n_steps; *out->n_remaining = n_remaining;
    if (n_peaks) {
        HIP_TRY(hipMemcpyAsync(out->peak_reads, d_preads, (size_t)n_peaks * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(out->peak_degree, d_pdeg, (size_t)n_peaks * 8, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipMemcpyAsync(out->removed_step, d_rstep, (size_t)R * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->removed_peak, d_rpeak, (size_t)R * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(d2h_staged(out->mapped, d_mapped, N, stream));
    if (out->score_left) HIP_TRY(d2h_staged(out->score_left, st.score, (size_t)N * 8, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return WEPP_OK;
}
