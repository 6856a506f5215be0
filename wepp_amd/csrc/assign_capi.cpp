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
#include <cstring>
#include <string>
#include <vector>

#include "assign.hpp"
#include "epp_host.hpp"
#include "handle.hpp"
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

namespace wepp {

int assign_check_selection(const wepp_epp_reads* rd, const void* out, uint32_t n_sel, const uint32_t* sel) {
    if (!rd || !out || (n_sel && !sel)) return set_error(WEPP_EINVAL, "null argument");
    if (n_sel == 0) return set_error(WEPP_EINVAL, "empty selection: n_sel must be at least 1");
    std::vector<uint32_t> sorted(sel, sel + n_sel);
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t k = 1; k < n_sel; k++)
        if (sorted[k] == sorted[k - 1])
            return set_error(WEPP_EINVAL, "haplotype " + std::to_string(sorted[k]) + " is selected more than once");
    return WEPP_OK;
}

int assign_check_handle(const wepp_mat_t* mat, const wepp_epp_reads* rd, uint32_t n_sel, const uint32_t* sel) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    const uint32_t R = rd->n_reads, N = mat->dev.N;
    for (uint32_t k = 0; k < n_sel; k++)
        if (sel[k] >= N)
            return set_error(WEPP_EINVAL, "sel[" + std::to_string(k) + "] = " + std::to_string(sel[k]) + " is not an arena index of this tree (" +
                                              std::to_string(N) + " haplotypes)");
    if (R && (!rd->read_off || !rd->start || !rd->end || !rd->degree)) return set_error(WEPP_EINVAL, "null read array");
    return WEPP_OK;
}

int assign_check_reads(const wepp_epp_reads* rd, uint32_t genome_size) {
    if (genome_size < 1) return set_error(WEPP_EINVAL, "genome_size must be at least 1");
    const uint32_t R = rd->n_reads;
    const uint64_t W = R ? rd->read_off[R] : 0;
    if (W && !rd->read_word) return set_error(WEPP_EINVAL, "null read_word");
    if (W >= (1ull << 32)) return set_error(WEPP_ELIMIT, "more than 2^32 read words in one call");
    return epp_validate_reads(rd, nullptr);
}

int assign_build_table(wepp_mat_t* mat, DevPool& pool, uint32_t K, const uint32_t* sel, hipStream_t stream, hipEvent_t begin,
                       hipEvent_t end, AssignTable* table) {
    const uint32_t Kp = assign_padded_cols(K);
    const uint32_t max_pos = mat->dev.max_pos;
    const uint64_t rows = (uint64_t)max_pos + 1;
    const uint64_t table_bytes = rows * Kp * 3;               // geno (1 B) + pre (2 B) per cell
    if (table_bytes > ASG_MAX_TABLE_BYTES)
        return set_error(WEPP_ELIMIT, "the genotype table of " + std::to_string(K) + " haplotypes over " + std::to_string(rows) +
                                          " positions needs " + std::to_string(table_bytes) + " bytes, more than 1 GiB: assign to the selection in parts");
    const uint32_t nblk = (uint32_t)((rows + ASG_SCAN_ROWS - 1) / ASG_SCAN_ROWS);
    hipError_t e;
#define GET(p, n) if ((e = pool.get(&p, (n))) != hipSuccess) return set_error(WEPP_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    uint32_t *d_sel, *d_bsum, *d_flag;
    uint8_t* d_geno;
    uint16_t* d_pre;
    GET(d_sel, K) GET(d_geno, rows * Kp) GET(d_pre, rows * Kp) GET(d_bsum, (size_t)nblk * Kp) GET(d_flag, 1)
#undef GET
    HIP_TRY(hipMemcpyAsync(d_sel, sel, (size_t)K * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(begin, stream));
    HIP_TRY(hipMemsetAsync(d_geno, 0, rows * Kp, stream));
    HIP_TRY(hipMemsetAsync(d_flag, 0, 4, stream));
    HIP_TRY(launch_assign_tables(mat->dev.node_woff, mat->dev.words, mat->dev.parent_dfs, d_sel, K, Kp, max_pos, d_geno, d_pre,
                                 d_bsum, d_flag, stream));
    uint32_t longest = 0;
    HIP_TRY(hipMemcpyAsync(&longest, d_flag, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(end, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (longest > ASG_MAX_PRE)
        return set_error(WEPP_ELIMIT, "a selected haplotype differs from the reference at " + std::to_string(longest) +
                                          " positions: the 16-bit prefix counts hold at most 65535");
    table->Kp = Kp; table->max_pos = max_pos; table->geno = d_geno; table->pre = d_pre;
    return WEPP_OK;
}

}  // namespace wepp

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
    const uint64_t W = R ? rd->read_off[R] : 0;

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
    const uint32_t max_pos = mat->dev.max_pos;
    const bool want_lists = out->asg_off != nullptr;

    HIP_TRY(hipSetDevice(mat->device));
    hipStream_t stream = nullptr;
    std::vector<uint32_t> order;
    epp_window_order(rd, order);

    DevPool pool(mat);
    hipError_t e;
#define GET(p, n) if ((e = pool.get(&p, (n))) != hipSuccess) return set_error(WEPP_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    uint32_t *d_off, *d_word, *d_order, *d_nepp, *d_sreads, *d_cover, *d_covered;
    int32_t *d_start, *d_end, *d_degree, *d_min;
    unsigned long long *d_sdeg, *d_ties = nullptr, *d_aoff = nullptr;
    GET(d_off, (size_t)R + 1) GET(d_word, W) GET(d_order, R) GET(d_start, R) GET(d_end, R) GET(d_degree, R)
    GET(d_min, R) GET(d_nepp, (size_t)R + 1) GET(d_sreads, Kp) GET(d_sdeg, Kp) GET(d_cover, (size_t)K * cover_words) GET(d_covered, K)
    if (want_lists) { GET(d_ties, (size_t)R * nslabs * 4) GET(d_aoff, (size_t)R + 1) }
    HIP_TRY(hipMemcpyAsync(d_off, rd->read_off, ((size_t)R + 1) * 4, hipMemcpyHostToDevice, stream));
    if (W) HIP_TRY(hipMemcpyAsync(d_word, rd->read_word, W * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_order, order.data(), (size_t)R * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_start, rd->start, (size_t)R * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_end, rd->end, (size_t)R * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_degree, rd->degree, (size_t)R * 4, hipMemcpyHostToDevice, stream));

    hipEvent_t ev[4];
    for (auto& x : ev) HIP_TRY(hipEventCreate(&x));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 4; i++) (void)hipEventDestroy(e[i]); } } evg{ev};

    // ---- the selection's genotype table --------------------------------------------------------------
    AssignTable tab;
    if (int rc = assign_build_table(mat, pool, K, sel, stream, ev[0], ev[1], &tab)) return rc;

    // ---- reads x selection ---------------------------------------------------------------------------
    HIP_TRY(hipMemsetAsync(d_sreads, 0, (size_t)Kp * 4, stream));
    HIP_TRY(hipMemsetAsync(d_sdeg, 0, (size_t)Kp * 8, stream));
    HIP_TRY(hipMemsetAsync(d_cover, 0, (size_t)K * cover_words * 4, stream));
    HIP_TRY(hipMemsetAsync(d_nepp + R, 0, 4, stream));
    AssignArgs a{};
    a.R = R; a.K = K; a.Kp = Kp; a.max_pos = max_pos; a.genome_size = genome_size; a.cover_words = cover_words;
    a.geno = tab.geno; a.pre = tab.pre;
    a.read_off = d_off; a.read_word = d_word; a.start = d_start; a.end = d_end; a.degree = d_degree; a.order = d_order;
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
        GET(d_temp, temp_bytes)
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
        GET(d_asel, need)
        HIP_TRY(launch_assign_lists(d_ties, d_aoff, R, Kp, d_asel, stream));
    }
    HIP_TRY(hipEventRecord(ev[3], stream));
    if (d_asel) HIP_TRY(d2h_staged(out->asg_sel, d_asel, need * 4, stream));
    HIP_TRY(hipStreamSynchronize(stream));
#undef GET
    g_last = AssignTiming{};
    (void)hipEventElapsedTime(&g_last.tables_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&g_last.assign_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&g_last.finish_ms, ev[2], ev[3]);
    if (short_lists)
        return set_error(WEPP_ELIMIT, "asg_sel holds " + std::to_string(out->asg_capacity) + " entries, " + std::to_string(need) +
                                          " needed: every other output is complete, call again with a buffer of asg_off[n_reads] entries");
    return WEPP_OK;
}
