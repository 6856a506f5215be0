// assign_capi.cpp -- wepp_epp_assign: host side of the read -> selected haplotype assignment
// (arena::dump_read2haplotype_mapping, src/WEPP/arena.cpp:590-696; the same loop in
// arena::resolve_unaccounted_mutations, :833-866).
//
// The reference runs reads x selected haplotypes merges of sorted lists (haplotype::mutation_distance,
// src/WEPP/haplotype.hpp:123-173) on the host.  Here the selection's genotypes become a position-major table
// on the device once per call, the reads are visited in window order and a wave scores one read against 256
// haplotypes per row load (assign_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "epp_host.hpp"
#include "staged_copy.hpp"

namespace {

struct AssignTiming { float tables_ms = 0, assign_ms = 0, finish_ms = 0; };
thread_local AssignTiming g_last;

}  // namespace

extern "C" int wepp_epp_assign_last_timing(double* tables_ms, double* assign_ms, double* finish_ms) {
    if (tables_ms) *tables_ms = g_last.tables_ms;
    if (assign_ms) *assign_ms = g_last.assign_ms;
    if (finish_ms) *finish_ms = g_last.finish_ms;
    return WEPP_OK;
}

extern "C" int wepp_epp_assign(wepp_mat_t* mat, const wepp_epp_reads* rd, uint32_t genome_size, uint32_t n_sel,
                               const uint32_t* sel, wepp_assign_out* out) {
    // the selection first: what can be said about it without the handle is said without it
    if (int rc = assign_check_selection(rd, out, n_sel, sel)) return rc;
    if (int rc = assign_check_handle(mat, rd, n_sel, sel)) return rc;
    const uint32_t R = rd->n_reads, K = n_sel;
    if ((R && (!out->min_dist || !out->n_epp)) || !out->sel_reads || !out->sel_degree || !out->sel_covered)
        return set_error(WEPP_EINVAL, "null output array");
    if ((out->asg_off == nullptr) != (out->asg_sel == nullptr) && !(out->asg_off && out->asg_capacity == 0))
        return set_error(WEPP_EINVAL, "asg_off and asg_sel go together");
    if (int rc = assign_check_reads(rd, genome_size)) return rc;

    const uint32_t cover_words = (uint32_t)(((uint64_t)genome_size + 31) / 32);
    if (R == 0) {
        std::fill(out->sel_reads, out->sel_reads + K, 0u);
        std::fill(out->sel_degree, out->sel_degree + K, (int64_t)0);
        std::fill(out->sel_covered, out->sel_covered + K, 0u);
        if (out->cover_bits) std::fill(out->cover_bits, out->cover_bits + (size_t)K * cover_words, 0u);
        if (out->asg_off) out->asg_off[0] = 0;
        return WEPP_OK;
    }

    const uint32_t Kp = assign_padded_cols(K), nslabs = Kp / ASG_SLAB;
    const bool want_lists = out->asg_off != nullptr;

    HIP_TRY(hipSetDevice(mat->device));
    hipStream_t stream = nullptr;
    std::vector<uint32_t> order;
    epp_window_order(rd, order);

    DevPool pool(mat->epp_cache);
    DevReads reads;
    if (int rc = upload_reads(pool, rd, order, stream, &reads)) return rc;
    uint32_t *d_nepp, *d_sreads, *d_cover, *d_covered;
    int32_t* d_min;
    unsigned long long *d_sdeg, *d_ties = nullptr, *d_aoff = nullptr;
    DEV_GET(pool, d_min, R); DEV_GET(pool, d_nepp, (size_t)R + 1); DEV_GET(pool, d_sreads, Kp); DEV_GET(pool, d_sdeg, Kp);
    DEV_GET(pool, d_cover, (size_t)K * cover_words); DEV_GET(pool, d_covered, K);
    if (want_lists) { DEV_GET(pool, d_ties, (size_t)R * nslabs * 4); DEV_GET(pool, d_aoff, (size_t)R + 1); }

    DevEvents<4> ev;
    if (int rc = ev.create()) return rc;

    // ---- the selection's genotype table --------------------------------------------------------------
    AssignTable tab;
    if (int rc = assign_build_table(mat, pool, K, sel, stream, ev[0], ev[1], &tab)) return rc;

    // ---- reads x selection ---------------------------------------------------------------------------
    HIP_TRY(hipMemsetAsync(d_sreads, 0, (size_t)Kp * 4, stream));
    HIP_TRY(hipMemsetAsync(d_sdeg, 0, (size_t)Kp * 8, stream));
    HIP_TRY(hipMemsetAsync(d_cover, 0, (size_t)K * cover_words * 4, stream));
    HIP_TRY(hipMemsetAsync(d_nepp + R, 0, 4, stream));
    AssignArgs a = assign_args(tab, K, reads);
    a.genome_size = genome_size; a.cover_words = cover_words;
    a.min_dist = d_min; a.n_epp = d_nepp; a.ties = d_ties;
    a.sel_reads = d_sreads; a.sel_degree = d_sdeg; a.cover = d_cover;
    HIP_TRY(launch_assign(a, stream));
    HIP_TRY(hipEventRecord(ev[2], stream));

    // ---- lists, coverage counts ------------------------------------------------------------------------
    HIP_TRY(launch_assign_popcount(d_cover, K, cover_words, d_covered, stream));
    if (want_lists) {
        size_t temp_bytes = 0;
        HIP_TRY(assign_scan_temp_bytes(R, &temp_bytes));
        char* d_temp;
        DEV_GET(pool, d_temp, temp_bytes);
        HIP_TRY(launch_assign_scan(d_nepp, d_aoff, R, d_temp, temp_bytes, stream));
        HIP_TRY(hipMemcpyAsync(out->asg_off, d_aoff, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipMemcpyAsync(out->min_dist, d_min, (size_t)R * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->n_epp, d_nepp, (size_t)R * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->sel_reads, d_sreads, (size_t)K * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->sel_degree, d_sdeg, (size_t)K * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->sel_covered, d_covered, (size_t)K * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (out->cover_bits) HIP_TRY(d2h_staged(out->cover_bits, d_cover, (size_t)K * cover_words * 4, stream));
    // the size of the lists is known now: too small a buffer leaves them out, everything else stands
    const uint64_t need = want_lists ? out->asg_off[R] : 0;
    const bool short_lists = want_lists && (need > out->asg_capacity || (need && !out->asg_sel));
    uint32_t* d_asel = nullptr;
    if (want_lists && need && !short_lists) {
        DEV_GET(pool, d_asel, need);
        HIP_TRY(launch_assign_lists(d_ties, d_aoff, R, Kp, d_asel, stream));
    }
    HIP_TRY(hipEventRecord(ev[3], stream));
    if (d_asel) HIP_TRY(d2h_staged(out->asg_sel, d_asel, need * 4, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    g_last = AssignTiming{};
    (void)hipEventElapsedTime(&g_last.tables_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&g_last.assign_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&g_last.finish_ms, ev[2], ev[3]);
    if (short_lists)
        return set_error(WEPP_ELIMIT, "asg_sel holds " + std::to_string(out->asg_capacity) + " entries, " + std::to_string(need) +
                                          " needed: every other output is complete, call again with a buffer of asg_off[n_reads] entries");
    return WEPP_OK;
}
