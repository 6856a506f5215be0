// epp_capi.cpp -- wepp_epp_map: host side of WEPP's own read placement
// (wepp_filter::cartesian_map, src/WEPP/initial_filter.cpp:140-239).
//
// The argument checks, the empty batch and the timing query; the sweep itself is epp_map_run (epp_sweep.cpp).
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

namespace {

struct EppTiming { float select_ms = 0, sweep1_ms = 0, sweep2_ms = 0, finish_ms = 0; uint64_t events_swept = 0, stream_events = 0; uint32_t groups = 0, jobs = 0; };
thread_local EppTiming g_last;

}  // namespace

extern "C" int wepp_mat_dfs_order(const wepp_mat_t* mat, uint32_t* ids) {
    if (!mat || !ids) return set_error(WEPP_EINVAL, "null argument");
    std::memcpy(ids, mat->dfs2id.data(), mat->dfs2id.size() * sizeof(uint32_t));
    return WEPP_OK;
}

extern "C" int wepp_epp_last_timing(double* select_ms, double* sweep1_ms, double* sweep2_ms, double* finish_ms,
                                    uint64_t* events_swept, uint64_t* stream_events, uint32_t* groups,
                                    uint32_t* jobs) {
    if (select_ms) *select_ms = g_last.select_ms;
    if (sweep1_ms) *sweep1_ms = g_last.sweep1_ms;
    if (sweep2_ms) *sweep2_ms = g_last.sweep2_ms;
    if (finish_ms) *finish_ms = g_last.finish_ms;
    if (events_swept) *events_swept = g_last.events_swept;
    if (stream_events) *stream_events = g_last.stream_events;
    if (groups) *groups = g_last.groups;
    if (jobs) *jobs = g_last.jobs;
    return WEPP_OK;
}

extern "C" int wepp_epp_map(wepp_mat_t* mat, const wepp_epp_reads* rd, uint32_t genome_size, uint32_t max_cached_epp,
                            wepp_epp_out* out) {
    if (!mat || !rd || !out) return set_error(WEPP_EINVAL, "null argument");
    const uint32_t R = rd->n_reads;
    const uint32_t N = mat->dev.N;
    if (R && (!rd->read_off || !rd->start || !rd->end || !rd->degree)) return set_error(WEPP_EINVAL, "null read array");
    if (!out->max_parsimony || !out->multiplicity || !out->hap_score) return set_error(WEPP_EINVAL, "null output array");
    if ((out->epp_off == nullptr) != (out->epp_nodes == nullptr)) return set_error(WEPP_EINVAL, "epp_off and epp_nodes go together");
    if (genome_size < EPP_BINS) return set_error(WEPP_EINVAL, "genome_size must be at least NUM_RANGE_BINS (50)");
    const uint64_t W = R ? rd->read_off[R] : 0;
    if (W && !rd->read_word) return set_error(WEPP_EINVAL, "null read_word");
    if (W >= (1ull << 32)) return set_error(WEPP_ELIMIT, "more than 2^32 read words in one call");

    // ---- validation (the reference's preconditions, made explicit) ----------------------
    long long total_degree = 0;
    if (int rc = epp_validate_reads(rd, &total_degree)) return rc;
    if (R == 0) {
        std::fill(out->hap_score, out->hap_score + N, 0.0);
        if (out->hap_read_counts) std::fill(out->hap_read_counts, out->hap_read_counts + (size_t)N * EPP_BINS, 0);
        if (out->hap_divergence) std::fill(out->hap_divergence, out->hap_divergence + N, std::nan(""));
        if (out->epp_off) out->epp_off[0] = 0;
        return WEPP_OK;
    }
    HIP_TRY(hipSetDevice(mat->device));
    // the sweep itself: epp_sweep.cpp (wepp_epp_peaks goes on from what it leaves on the device)
    DevPool pool(mat->epp_cache);
    EppMapState st;
    const int rc = epp_map_run(mat, pool, rd, genome_size, max_cached_epp, total_degree, out, false, &st);
    if (rc != WEPP_OK && !st.diff_score) return rc;        // (a short list buffer reports at the end of a complete call)
    g_last = EppTiming{};
    g_last.select_ms = st.select_ms; g_last.sweep1_ms = st.sweep1_ms; g_last.sweep2_ms = st.sweep2_ms; g_last.finish_ms = st.finish_ms;
    g_last.events_swept = st.sweep.events_swept;
    g_last.stream_events = st.sweep.stream_events;
    g_last.groups = st.groups;
    g_last.jobs = st.jobs;
    return rc;
}

// the EPP lists of the handle's last wepp_epp_map that did not fit the caller's buffer (nothing is computed again)
extern "C" int wepp_epp_fetch_lists(wepp_mat_t* mat, uint32_t* epp_nodes, uint64_t capacity) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    if (mat->epp_pending.empty()) return set_error(WEPP_EINVAL, "no EPP lists are pending on this handle");
    if (capacity < mat->epp_pending.size())
        return set_error(WEPP_ELIMIT, "epp_nodes holds " + std::to_string(capacity) + " entries, " + std::to_string(mat->epp_pending.size()) + " needed");
    if (!epp_nodes) return set_error(WEPP_EINVAL, "null argument");
    std::memcpy(epp_nodes, mat->epp_pending.data(), mat->epp_pending.size() * 4);
    std::vector<uint32_t>().swap(mat->epp_pending);
    return WEPP_OK;
}
