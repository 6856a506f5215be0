// sam_subsample_capi.cpp -- wepp_sam_build_subsampled: host side of sam::subsample in front of sam::build
// (src/WEPP/sam2pb.cpp:362-454) for reads that are already aligned strings.
//
// full pile-up -> keep table of the FULL table -> thresholds of all trials (radix select, six digit passes) -> the
// tiles' read lists -> per pass of trials: trial pile-up, divergence -> argmin -> flags, scan, the kept reads as a
// batch of their own -> the stages of wepp_sam_build behind the keep table (sam_host.hpp), unchanged.
//
// Departures from the reference, all stated in include/wepp_place.h: the draw is a seeded hash order (the reference
// shuffles with an mt19937 seeded from std::random_device and has no defined result), and among trials of equal
// divergence the lowest wins (the reference's winner among equals depends on thread timing).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "epp_host.hpp"
#include "sam.hpp"
#include "sam_host.hpp"
#include "sam_subsample.hpp"
#include "staged_copy.hpp"

namespace {

struct SubTiming { double select_ms = 0, trials_ms = 0, pick_ms = 0; };
thread_local SubTiming g_sub_last;

}  // namespace

extern "C" int wepp_sam_subsample_last_timing(double* select_ms, double* trials_ms, double* pick_ms) {
    if (select_ms) *select_ms = g_sub_last.select_ms;
    if (trials_ms) *trials_ms = g_sub_last.trials_ms;
    if (pick_ms) *pick_ms = g_sub_last.pick_ms;
    return WEPP_OK;
}

extern "C" int wepp_sam_build_subsampled(int device, const uint8_t* reference, uint32_t genome_size, const wepp_sam_reads* rd,
                                         const wepp_sam_params* par, const wepp_sam_subsample_params* sub, wepp_sam_out* out,
                                         wepp_sam_subsample_out* so) {
    using u64 = unsigned long long;
    if (int rc = sam_check_arguments(reference, genome_size, rd, par, out)) return rc;
    if (!sub || !so) return set_error(WEPP_EINVAL, "null argument");
    if (sub->max_reads == 0) return set_error(WEPP_EINVAL, "max_reads is 0");
    if (sub->trials == 0) return set_error(WEPP_EINVAL, "trials is 0");
    if (sub->trials > SUB_MAX_TRIALS) return set_error(WEPP_ELIMIT, "more than " + std::to_string(SUB_MAX_TRIALS) + " trials");
    const uint32_t R = rd->n_reads, m = sub->max_reads, T = sub->trials;
    if (!so->n_kept || !so->best_trial || (R && !so->kept)) return set_error(WEPP_EINVAL, "null output array");
    g_sub_last = SubTiming{};
    if (R <= m) {
        // nothing is drawn: the call is wepp_sam_build
        const int rc = wepp_sam_build(device, reference, genome_size, rd, par, out);
        *so->n_kept = R;
        for (uint32_t r = 0; r < R; r++) so->kept[r] = r;
        *so->best_trial = UINT32_MAX;
        if (so->divergence) std::fill(so->divergence, so->divergence + T, 0.0);
        if (so->threshold) std::fill(so->threshold, so->threshold + T, (uint64_t)0);
        return rc;
    }
    sam_reset_thread_state();
    const size_t cells = (size_t)genome_size * 6;
    const uint64_t B = rd->base_off[R];
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(WEPP_EDEVICE, "no HIP device found (wepp_place has no CPU fallback)");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = nullptr;

    wepp_mat::DevBlockCache cache;             // (declared before the pool: the pool hands its blocks back first)
    DevPool pool(cache);
    DevEvents<6> ev;                           // the phases of wepp_sam_last_timing (sam_finish)
    DevEvents<4> sev;                          // select | trials | pick
    if (int rc = ev.create()) return rc;
    if (int rc = sev.create()) return rc;

    // the bound of a pass of trials: read once per call; the environment only ever lowers it
    u64 pass_bytes = SUB_PASS_BYTES;
    if (const char* s = std::getenv("WEPP_SAM_SUBSAMPLE_PASS_BYTES")) {
        const u64 v = std::strtoull(s, nullptr, 10);
        if (v > 0) pass_bytes = std::min<u64>(v, SUB_PASS_BYTES);
    }
    // whole batches, at least one, at most 8192 trials (the launch's third grid dimension stays far below its limit)
    const u64 table_bytes = (u64)cells * 4;
    u64 per_pass = pass_bytes / table_bytes / SUB_BATCH * SUB_BATCH;
    per_pass = std::min<u64>(std::max<u64>(per_pass, SUB_BATCH), 8192);
    const uint32_t pass_trials = (uint32_t)std::min<u64>(per_pass, T);

    // ---- the reads and the reference on the device --------------------------------------------------------------
    const uint32_t tiles = (genome_size + SUB_TILE - 1) / SUB_TILE;
    const uint32_t select_trials = std::min(T, SUB_SELECT_TRIALS);
    uint8_t *d_ref, *d_base, *d_keep;
    uint32_t *d_start, *d_freq, *d_bad, *d_rank, *d_hist, *d_tcount, *d_cov, *d_tables, *d_best, *d_flag;
    u64 *d_boff, *d_hash, *d_thr, *d_toff, *d_foff;
    double* d_div;
    DEV_GET(pool, d_ref, genome_size); DEV_GET(pool, d_base, B); DEV_GET(pool, d_keep, cells); DEV_GET(pool, d_start, R);
    DEV_GET(pool, d_freq, cells); DEV_GET(pool, d_bad, 1); DEV_GET(pool, d_boff, (size_t)R + 1);
    DEV_GET(pool, d_hash, T); DEV_GET(pool, d_thr, T); DEV_GET(pool, d_rank, T); DEV_GET(pool, d_hist, (size_t)select_trials * SUB_BINS);
    DEV_GET(pool, d_tcount, (size_t)tiles + 1); DEV_GET(pool, d_toff, (size_t)tiles + 1); DEV_GET(pool, d_cov, 1);
    DEV_GET(pool, d_tables, (size_t)pass_trials * cells); DEV_GET(pool, d_div, T); DEV_GET(pool, d_best, 1);
    DEV_GET(pool, d_flag, (size_t)R + 1); DEV_GET(pool, d_foff, (size_t)R + 1);
    size_t scan_bytes = 0, scan_tiles = 0;
    HIP_TRY(sam_scan_temp_bytes(R, &scan_bytes));
    HIP_TRY(sam_scan_temp_bytes(tiles, &scan_tiles));
    scan_bytes = std::max(scan_bytes, scan_tiles);
    char* d_temp;
    DEV_GET(pool, d_temp, scan_bytes);
    std::vector<u64> trial_hash(T);
    for (uint32_t t = 0; t < T; t++) trial_hash[t] = sub_hash(sub->seed ^ sub_hash(t));
    const std::vector<uint32_t> rank0(T, m - 1);
    HIP_TRY(hipMemcpyAsync(d_ref, reference, genome_size, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_start, rd->start, (size_t)R * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_boff, rd->base_off, ((size_t)R + 1) * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_base, rd->base, B, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_hash, trial_hash.data(), (size_t)T * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_rank, rank0.data(), (size_t)T * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_thr, 0, (size_t)T * 8, stream));
    HIP_TRY(hipMemsetAsync(d_freq, 0, cells * 4, stream));
    HIP_TRY(hipMemsetAsync(d_bad, 0, 4, stream));
    HIP_TRY(hipMemsetAsync(d_cov, 0, 4, stream));
    HIP_TRY(hipMemsetAsync(d_tcount, 0, ((size_t)tiles + 1) * 4, stream));
    SamReadsDev reads{R, d_start, d_boff, d_base, d_ref, genome_size};

    // ---- the full table and its keep table -------------------------------------------------------------------------
    HIP_TRY(hipEventRecord(ev[0], stream));
    HIP_TRY(launch_sam_pileup(reads, d_freq, d_bad, stream));
    HIP_TRY(launch_sam_keep(d_freq, genome_size, par->min_af, par->min_depth, d_keep, stream));
    HIP_TRY(hipEventRecord(ev[1], stream));
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (bad) return set_error(WEPP_EINVAL, "a base byte is not one of 0..5 (ACGTN_)");

    // ---- thresholds: the m-th smallest key of every trial, digit by digit --------------------------------------------
    HIP_TRY(hipEventRecord(sev[0], stream));
    for (uint32_t g0 = 0; g0 < T; g0 += select_trials) {
        const uint32_t ng = std::min(select_trials, T - g0);
        for (uint32_t top = 64; top > 0;) {
            const uint32_t width = top >= SUB_DIGIT_BITS ? SUB_DIGIT_BITS : top, shift = top - width;   // 11 11 11 11 11 9
            HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)ng * SUB_BINS * 4, stream));
            HIP_TRY(launch_sub_histogram(d_hash + g0, d_thr + g0, ng, R, shift, width, top == 64, d_hist, stream));
            HIP_TRY(launch_sub_pick_digit(d_hist, ng, width, d_thr + g0, d_rank + g0, stream));
            top = shift;
        }
    }
    HIP_TRY(hipEventRecord(sev[1], stream));

    // ---- the tiles' read lists ---------------------------------------------------------------------------------------
    HIP_TRY(launch_sub_bin_count(reads, d_tcount, stream));
    HIP_TRY(launch_sam_scan(d_tcount, d_toff, tiles, d_temp, scan_bytes, stream));
    std::vector<uint32_t> tile_count(tiles);
    HIP_TRY(hipMemcpyAsync(tile_count.data(), d_tcount, (size_t)tiles * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    u64 list_len = 0;
    uint32_t longest = 0;
    for (uint32_t c : tile_count) { list_len += c; longest = std::max(longest, c); }
    if (list_len < R || list_len > (u64)R + B) return set_error(WEPP_EDEVICE, "the tiles' read lists hold " + std::to_string(list_len) + " entries");
    uint32_t* d_list;
    DEV_GET(pool, d_list, (size_t)list_len);
    HIP_TRY(hipMemsetAsync(d_tcount, 0, ((size_t)tiles + 1) * 4, stream));
    HIP_TRY(launch_sub_bin_fill(reads, d_toff, d_tcount, d_list, stream));
    HIP_TRY(launch_sub_covered(d_freq, genome_size, d_cov, stream));

    // ---- the trials, a pass of whole batches at a time ---------------------------------------------------------------
    for (uint32_t t0 = 0; t0 < T; t0 += pass_trials) {
        const uint32_t nt = std::min(pass_trials, T - t0);
        HIP_TRY(hipMemsetAsync(d_tables, 0, (size_t)nt * cells * 4, stream));
        HIP_TRY(launch_sub_pileup(reads, d_toff, d_list, longest, d_hash, d_thr, t0, nt, d_tables, stream));
        HIP_TRY(launch_sub_divergence(d_freq, d_cov, genome_size, d_tables, t0, nt, d_div, stream));
    }
    HIP_TRY(hipEventRecord(sev[2], stream));

    // ---- pick and compaction -----------------------------------------------------------------------------------------
    HIP_TRY(launch_sub_argmin(d_div, T, d_best, stream));
    HIP_TRY(hipMemsetAsync(d_flag + R, 0, 4, stream));
    HIP_TRY(launch_sub_flags(R, d_hash, d_thr, d_best, d_flag, stream));
    HIP_TRY(launch_sam_scan(d_flag, d_foff, R, d_temp, scan_bytes, stream));
    u64 n_kept64 = 0;
    uint32_t best = 0;
    HIP_TRY(hipMemcpyAsync(&n_kept64, d_foff + R, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&best, d_best, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (best >= T) return set_error(WEPP_EDEVICE, "no trial was picked");
    if (n_kept64 != m) return set_error(WEPP_EDEVICE, "trial " + std::to_string(best) + " keeps " + std::to_string(n_kept64) + " reads, not " + std::to_string(m));
    uint32_t *d_kept, *d_kstart, *d_klen;
    u64* d_koff;
    DEV_GET(pool, d_kept, m); DEV_GET(pool, d_kstart, m); DEV_GET(pool, d_klen, (size_t)m + 1); DEV_GET(pool, d_koff, (size_t)m + 1);
    HIP_TRY(hipMemsetAsync(d_klen + m, 0, 4, stream));
    HIP_TRY(launch_sub_kept(reads, d_flag, d_foff, d_kept, d_kstart, d_klen, stream));
    HIP_TRY(launch_sam_scan(d_klen, d_koff, m, d_temp, scan_bytes, stream));
    u64 kept_columns = 0;
    HIP_TRY(hipMemcpyAsync(&kept_columns, d_koff + m, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (kept_columns == 0 || kept_columns > B) return set_error(WEPP_EDEVICE, "the kept reads hold " + std::to_string(kept_columns) + " columns");
    uint8_t* d_kbase;
    DEV_GET(pool, d_kbase, (size_t)kept_columns);
    HIP_TRY(launch_sub_gather(reads, m, d_kept, d_koff, d_kbase, stream));
    HIP_TRY(hipEventRecord(sev[3], stream));

    *so->n_kept = m;
    *so->best_trial = best;
    HIP_TRY(d2h_staged(so->kept, d_kept, (size_t)m * 4, stream));
    if (so->divergence) HIP_TRY(hipMemcpyAsync(so->divergence, d_div, (size_t)T * 8, hipMemcpyDeviceToHost, stream));
    if (so->threshold) HIP_TRY(hipMemcpyAsync(so->threshold, d_thr, (size_t)T * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3; i++) HIP_TRY(hipEventElapsedTime(&ms[i], sev[i], sev[i + 1]));
    g_sub_last.select_ms = ms[0]; g_sub_last.trials_ms = ms[1]; g_sub_last.pick_ms = ms[2];

    // ---- correction (under the FULL table's keep table), sort and merge of the kept reads ------------------------------
    SamScratch scratch;
    if (int rc = sam_get_scratch(pool, m, &scratch)) return rc;
    const SamReadsDev kept_reads{m, d_kstart, d_koff, d_kbase, d_ref, genome_size};
    return sam_finish(pool, stream, kept_reads, kept_columns, d_keep, d_freq, nullptr, scratch, ev.ev, so->kept, out);
}
