// resolve_capi.cpp -- wepp_epp_resolve: host side of the attribution of residual mutations to selected
// haplotypes (arena::resolve_unaccounted_mutations, src/WEPP/arena.cpp:739-892).
//
// The reference copies every read under every residual mutation it touches and runs the reads x selected
// haplotypes loop of mutation_distance per copy.  Here the reads are marked once (resolve_kernels.hip), the
// touched ones go through k_assign once as a device-resident batch, and a tally over the relation lists turns
// their tie masks into per-mutation counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "epp_host.hpp"
#include "resolve.hpp"
#include "resolve_host.hpp"
#include "staged_copy.hpp"

namespace {

struct ResolveTiming { float mark_ms = 0, tables_ms = 0, assign_ms = 0, tally_ms = 0; };
thread_local ResolveTiming g_last;

void zero_outputs(wepp_resolve_out* out, uint32_t M, uint32_t K) {
    const size_t KW = (K + 31) / 32;
    if (out->rel_off) std::fill(out->rel_off, out->rel_off + (size_t)M + 1, (uint64_t)0);
    std::fill(out->n_covered, out->n_covered + M, 0u);
    std::fill(out->n_masked, out->n_masked + M, 0u);
    std::fill(out->best_degree, out->best_degree + M, (int64_t)0);
    std::fill(out->best_mask, out->best_mask + (size_t)M * KW, 0u);
    if (out->hap_reads) std::fill(out->hap_reads, out->hap_reads + (size_t)M * K, 0u);
    if (out->hap_degree) std::fill(out->hap_degree, out->hap_degree + (size_t)M * K, (int64_t)0);
    *out->n_touched = 0;
}

}  // namespace

extern "C" int wepp_epp_resolve_last_timing(double* mark_ms, double* tables_ms, double* assign_ms, double* tally_ms) {
    if (mark_ms) *mark_ms = g_last.mark_ms;
    if (tables_ms) *tables_ms = g_last.tables_ms;
    if (assign_ms) *assign_ms = g_last.assign_ms;
    if (tally_ms) *tally_ms = g_last.tally_ms;
    return WEPP_OK;
}

extern "C" int wepp_epp_resolve(wepp_mat_t* mat, const wepp_epp_reads* rd, uint32_t genome_size, uint32_t n_sel,
                                const uint32_t* sel, uint32_t n_res, const uint32_t* res_word, wepp_resolve_out* out) {
    if (int rc = assign_check_selection(rd, out, n_sel, sel)) return rc;
    if (n_res && !res_word) return set_error(WEPP_EINVAL, "null argument");
    if (int rc = assign_check_handle(mat, rd, n_sel, sel)) return rc;
    const uint32_t R = rd->n_reads, K = n_sel, M = n_res;
    if (!out->n_touched || (M && (!out->n_covered || !out->n_masked || !out->best_degree || !out->best_mask)))
        return set_error(WEPP_EINVAL, "null output array");
    if ((out->rel_off == nullptr) != (out->rel_read == nullptr) && !(out->rel_off && out->rel_capacity == 0))
        return set_error(WEPP_EINVAL, "rel_off and rel_read go together");
    if (int rc = assign_check_reads(rd, genome_size)) return rc;
    if (R >= (1u << 31)) return set_error(WEPP_ELIMIT, "2^31 or more reads in one call: bit 31 of rel_read marks a masked read");
    if (int rc = resolve_check_residual(M, res_word, genome_size)) return rc;
    g_last = ResolveTiming{};
    if (M == 0 || R == 0) {
        zero_outputs(out, M, K);
        return WEPP_OK;
    }
    const uint32_t KW = (K + 31) / 32;
    const bool want_lists = out->rel_off != nullptr;

    std::vector<uint32_t> res_pos, res_sorted, res_idx, order;
    resolve_sort_residual(M, res_word, res_pos, res_sorted, res_idx);
    epp_window_order(rd, order);

    HIP_TRY(hipSetDevice(mat->device));
    hipStream_t stream = nullptr;
    DevPool pool(mat->epp_cache);
    DevReads reads, touched;
    if (int rc = upload_reads(pool, rd, order, stream, &reads)) return rc;
    uint32_t *d_rpos, *d_rword, *d_ridx, *d_counts, *d_ncov, *d_nmask;
    unsigned long long* d_scans;
    const size_t R1 = (size_t)R + 1;
    DEV_GET(pool, d_rpos, M); DEV_GET(pool, d_rword, M); DEV_GET(pool, d_ridx, M); DEV_GET(pool, d_counts, 4 * R1);
    DEV_GET(pool, d_scans, 4 * R1); DEV_GET(pool, d_ncov, M); DEV_GET(pool, d_nmask, M);
    HIP_TRY(hipMemcpyAsync(d_rpos, res_pos.data(), (size_t)M * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_rword, res_sorted.data(), (size_t)M * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_ridx, res_idx.data(), (size_t)M * 4, hipMemcpyHostToDevice, stream));

    DevEvents<6> ev;
    if (int rc = ev.create()) return rc;
    HIP_TRY(hipEventRecord(ev[0], stream));

    // ---- mark: count, scans ------------------------------------------------------------------------------
    MarkArgs ma{};
    ma.R = R; ma.M = M;
    ma.res_pos = d_rpos; ma.res_word = d_rword; ma.res_idx = d_ridx;
    ma.read_off = reads.read_off; ma.read_word = reads.read_word; ma.start = reads.start; ma.end = reads.end; ma.degree = reads.degree; ma.order = reads.order;
    ma.n_rel = d_counts; ma.n_words = d_counts + R1; ma.touched = d_counts + 2 * R1; ma.touched_place = d_counts + 3 * R1;
    ma.rel_at = d_scans; ma.word_at = d_scans + R1; ma.compact = d_scans + 2 * R1; ma.place_at = d_scans + 3 * R1;
    HIP_TRY(hipMemsetAsync(d_counts, 0, 4 * R1 * 4, stream));       // (the R-th element of each: the scans' totals)
    HIP_TRY(hipMemsetAsync(d_ncov, 0, (size_t)M * 4, stream));
    HIP_TRY(hipMemsetAsync(d_nmask, 0, (size_t)M * 4, stream));
    HIP_TRY(launch_resolve_count(ma, stream));
    {
        size_t temp_bytes = 0;
        HIP_TRY(assign_scan_temp_bytes(R, &temp_bytes));
        char* d_temp;
        DEV_GET(pool, d_temp, temp_bytes);
        for (int i = 0; i < 4; i++)
            HIP_TRY(launch_assign_scan(d_counts + i * R1, d_scans + i * R1, R, d_temp, temp_bytes, stream));
    }
    unsigned long long totals[3] = {0, 0, 0};    // relations, entries of the touched reads, touched reads
    for (int i = 0; i < 3; i++)
        HIP_TRY(hipMemcpyAsync(&totals[i], d_scans + i * R1 + R, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t n_rel = totals[0], W2 = totals[1];
    const uint32_t T = (uint32_t)totals[2];
    if (T == 0) {
        zero_outputs(out, M, K);
        return WEPP_OK;
    }
    if (W2 >= (1ull << 32)) return set_error(WEPP_ELIMIT, "more than 2^32 read words in the touched reads after the insertions");

    // ---- mark: the touched reads as a batch, the relations mutation-major ---------------------------------------
    uint32_t *d_key, *d_val, *d_key2, *d_val2;
    unsigned long long* d_reloff;
    if (int rc = alloc_reads(pool, T, W2, &touched)) return rc;
    DEV_GET(pool, d_key, n_rel); DEV_GET(pool, d_val, n_rel); DEV_GET(pool, d_key2, n_rel); DEV_GET(pool, d_val2, n_rel);
    DEV_GET(pool, d_reloff, (size_t)M + 1);
    ma.out_off = touched.read_off; ma.out_word = touched.read_word; ma.out_start = touched.start; ma.out_end = touched.end;
    ma.out_degree = touched.degree; ma.out_order = touched.order; ma.rel_key = d_key; ma.rel_val = d_val; ma.n_covered = d_ncov; ma.n_masked = d_nmask;
    HIP_TRY(launch_resolve_write(ma, stream));
    {
        uint32_t key_bits = 1;
        while (key_bits < 32 && (1ull << key_bits) < M) key_bits++;
        size_t temp_bytes = 0;
        HIP_TRY(resolve_sort_temp_bytes(n_rel, key_bits, &temp_bytes));
        char* d_temp;
        DEV_GET(pool, d_temp, temp_bytes);
        HIP_TRY(launch_resolve_sort(d_key, d_key2, d_val, d_val2, n_rel, key_bits, d_temp, temp_bytes, stream));
    }
    HIP_TRY(launch_resolve_offsets(d_key2, n_rel, M, d_reloff, stream));
    std::vector<uint64_t> rel_off_own;
    uint64_t* rel_off = out->rel_off;
    if (!rel_off) { rel_off_own.resize((size_t)M + 1); rel_off = rel_off_own.data(); }
    HIP_TRY(hipMemcpyAsync(rel_off, d_reloff, ((size_t)M + 1) * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(ev[1], stream));

    // ---- the selection's genotype table, the touched reads x selection ----------------------------------------
    AssignTable tab;
    if (int rc = assign_build_table(mat, pool, K, sel, stream, ev[2], ev[3], &tab)) return rc;
    const uint32_t Kp = tab.Kp, nslabs = Kp / ASG_SLAB;
    uint32_t *d_nepp, *d_sreads, *d_cover, *d_hreads, *d_bmask;
    int32_t* d_min;
    unsigned long long *d_sdeg, *d_ties, *d_hdeg;
    long long* d_bdeg;
    DEV_GET(pool, d_min, T); DEV_GET(pool, d_nepp, (size_t)T + 1); DEV_GET(pool, d_sreads, Kp); DEV_GET(pool, d_sdeg, Kp); DEV_GET(pool, d_cover, 0);
    DEV_GET(pool, d_ties, (size_t)T * nslabs * 4); DEV_GET(pool, d_hreads, (size_t)M * K); DEV_GET(pool, d_hdeg, (size_t)M * K);
    DEV_GET(pool, d_bdeg, M); DEV_GET(pool, d_bmask, (size_t)M * KW);
    HIP_TRY(hipMemsetAsync(d_sreads, 0, (size_t)Kp * 4, stream));
    HIP_TRY(hipMemsetAsync(d_sdeg, 0, (size_t)Kp * 8, stream));
    // genome_size 0: no site is inside the genome, so k_assign sets no coverage bit and never looks at `cover` (0 elements);
    // min_dist, n_epp, sel_reads and sel_degree are scratch here, the tie masks are what is wanted
    AssignArgs a = assign_args(tab, K, touched);
    a.genome_size = 0; a.cover_words = 0;
    a.min_dist = d_min; a.n_epp = d_nepp; a.ties = d_ties;
    a.sel_reads = d_sreads; a.sel_degree = d_sdeg; a.cover = d_cover;
    HIP_TRY(launch_assign(a, stream));
    HIP_TRY(hipEventRecord(ev[4], stream));

    // ---- tally, best ------------------------------------------------------------------------------------------
    uint64_t longest = 0;                       // (rel_off arrived with the table's synchronisation)
    for (uint32_t m = 0; m < M; m++) longest = std::max(longest, rel_off[m + 1] - rel_off[m]);
    HIP_TRY(hipMemsetAsync(d_hreads, 0, (size_t)M * K * 4, stream));
    HIP_TRY(hipMemsetAsync(d_hdeg, 0, (size_t)M * K * 8, stream));
    TallyArgs ta{};
    ta.M = M; ta.K = K; ta.Kp = Kp;
    ta.rel_off = d_reloff; ta.rel_read = d_val2; ta.compact = ma.compact; ta.degree = touched.degree; ta.ties = d_ties;
    ta.hap_reads = d_hreads; ta.hap_degree = d_hdeg;
    HIP_TRY(launch_resolve_tally(ta, (longest + RES_CHUNK - 1) / RES_CHUNK, stream));
    HIP_TRY(launch_resolve_best(d_hreads, d_hdeg, M, K, d_bdeg, d_bmask, stream));
    HIP_TRY(hipEventRecord(ev[5], stream));

    HIP_TRY(hipMemcpyAsync(out->n_covered, d_ncov, (size_t)M * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->n_masked, d_nmask, (size_t)M * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->best_degree, d_bdeg, (size_t)M * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->best_mask, d_bmask, (size_t)M * KW * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (out->hap_reads) HIP_TRY(d2h_staged(out->hap_reads, d_hreads, (size_t)M * K * 4, stream));
    if (out->hap_degree) HIP_TRY(d2h_staged(out->hap_degree, d_hdeg, (size_t)M * K * 8, stream));
    *out->n_touched = T;
    // too small a buffer leaves the lists out, everything else stands
    const bool short_lists = want_lists && (n_rel > out->rel_capacity || !out->rel_read);
    if (want_lists && !short_lists) HIP_TRY(d2h_staged(out->rel_read, d_val2, n_rel * 4, stream));
    (void)hipEventElapsedTime(&g_last.mark_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&g_last.tables_ms, ev[2], ev[3]);
    (void)hipEventElapsedTime(&g_last.assign_ms, ev[3], ev[4]);
    (void)hipEventElapsedTime(&g_last.tally_ms, ev[4], ev[5]);
    if (short_lists)
        return set_error(WEPP_ELIMIT, "rel_read holds " + std::to_string(out->rel_capacity) + " entries, " + std::to_string(n_rel) +
                                          " needed: every other output is complete, call again with a buffer of rel_off[n_res] entries");
    return WEPP_OK;
}
