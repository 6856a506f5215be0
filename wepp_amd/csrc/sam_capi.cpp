// sam_capi.cpp -- wepp_sam_build: host side of sam::build (src/WEPP/sam2pb.cpp:262-275, 281-314, 456-470) for reads
// that are already aligned strings (the parse is the host mirror's, wepp_amd/host/sam_reader.cpp).
//
// pile-up -> keep table -> word counts -> scan -> words -> merge sort of the read indices -> heads -> scan -> groups ->
// scan of the leaders' word counts -> merged batch.  The call takes no tree handle: its device blocks come from a
// cache of its own that lives as long as the call.
//
// Departures from the reference, all stated in include/wepp_place.h: the earliest input read leads a group of equal
// reads (the reference's unstable sort leaves it open), subsampling is a call of its own with a defined draw
// (wepp_sam_build_subsampled, sam_subsample_capi.cpp; this call takes every read it is given), and inputs on which
// the reference would index outside its tables are WEPP_EINVAL.
//
// The argument checks and the stages behind the keep table are routines (sam_host.hpp) that the subsampled call runs
// too, over the reads it keeps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "epp_host.hpp"
#include "sam.hpp"
#include "sam_host.hpp"
#include "staged_copy.hpp"

namespace {

struct SamTiming { double pileup_ms = 0, correct_ms = 0, sort_ms = 0, merge_ms = 0; };
thread_local SamTiming g_last;
thread_local std::vector<uint32_t> g_pending;      // the merged reads' words that did not fit the caller's buffer
thread_local bool g_have_pending = false;

int check_reads(const wepp_sam_reads* rd, uint32_t genome_size) {
    const uint32_t R = rd->n_reads;
    if (rd->base_off[0] != 0) return set_error(WEPP_EINVAL, "base_off[0] is not 0");
    for (uint32_t r = 0; r < R; r++) {
        const uint64_t lo = rd->base_off[r], hi = rd->base_off[r + 1];
        if (hi < lo) return set_error(WEPP_EINVAL, "base_off does not ascend at read " + std::to_string(r));
        if (hi == lo) return set_error(WEPP_EINVAL, "read " + std::to_string(r) + " is empty");
        if (rd->start[r] >= genome_size || hi - lo > (uint64_t)genome_size - rd->start[r])
            return set_error(WEPP_EINVAL, "read " + std::to_string(r) + " (start " + std::to_string(rd->start[r]) + ", " + std::to_string(hi - lo) +
                                              " columns) does not lie inside [0, " + std::to_string(genome_size) + ")");
    }
    return WEPP_OK;
}

}  // namespace

extern "C" int wepp_sam_last_timing(double* pileup_ms, double* correct_ms, double* sort_ms, double* merge_ms) {
    if (pileup_ms) *pileup_ms = g_last.pileup_ms;
    if (correct_ms) *correct_ms = g_last.correct_ms;
    if (sort_ms) *sort_ms = g_last.sort_ms;
    if (merge_ms) *merge_ms = g_last.merge_ms;
    return WEPP_OK;
}

extern "C" int wepp_sam_fetch_words(uint32_t* read_word, uint64_t capacity) {
    if (!g_have_pending) return set_error(WEPP_EINVAL, "no read words are pending in this thread");
    if (capacity < g_pending.size())
        return set_error(WEPP_ELIMIT, "read_word holds " + std::to_string(capacity) + " entries, " + std::to_string(g_pending.size()) + " needed");
    if (!g_pending.empty() && !read_word) return set_error(WEPP_EINVAL, "null read_word");
    if (!g_pending.empty()) std::memcpy(read_word, g_pending.data(), g_pending.size() * 4);
    std::vector<uint32_t>().swap(g_pending);
    g_have_pending = false;
    return WEPP_OK;
}

namespace wepp {

int sam_check_arguments(const uint8_t* reference, uint32_t genome_size, const wepp_sam_reads* rd, const wepp_sam_params* par, const wepp_sam_out* out) {
    if (!rd || !par || !out || (genome_size && !reference)) return set_error(WEPP_EINVAL, "null argument");
    const uint32_t R = rd->n_reads;
    if (!out->n_merged || !out->group_off || !out->read_off || (R && (!out->order || !out->start || !out->end || !out->degree)))
        return set_error(WEPP_EINVAL, "null output array");
    if (out->word_capacity && !out->read_word) return set_error(WEPP_EINVAL, "null read_word with a capacity");
    if (R && (!rd->start || !rd->base_off || !rd->base)) return set_error(WEPP_EINVAL, "null read array");
    if (genome_size > WEPP_MAX_POSITION) return set_error(WEPP_ELIMIT, "genome_size exceeds the 20-bit positions of a read word");
    if (R >= (1u << 31)) return set_error(WEPP_ELIMIT, "2^31 or more reads in one call");
    if (R) if (int rc = check_reads(rd, genome_size)) return rc;
    return WEPP_OK;
}

void sam_reset_thread_state() {
    g_last = SamTiming{};
    std::vector<uint32_t>().swap(g_pending);
    g_have_pending = false;
}

int sam_get_scratch(DevPool& pool, uint32_t R, SamScratch* s) {
    DEV_GET(pool, s->n_words, (size_t)R + 1);
    DEV_GET(pool, s->word_off, (size_t)R + 1);
    HIP_TRY(sam_scan_temp_bytes(R, &s->scan_bytes));
    HIP_TRY(sam_sort_temp_bytes(R, &s->sort_bytes));
    DEV_GET(pool, s->temp, std::max(s->scan_bytes, s->sort_bytes));
    return WEPP_OK;
}

int sam_finish(DevPool& pool, hipStream_t stream, const SamReadsDev& reads, uint64_t B, const uint8_t* d_keep, const uint32_t* d_freq,
               const uint32_t* d_bad, const SamScratch& scratch, const hipEvent_t* ev, const uint32_t* order_map, wepp_sam_out* out) {
    const uint32_t R = reads.R, genome_size = reads.G;
    const size_t cells = (size_t)genome_size * 6;
    uint32_t* const d_nwords = scratch.n_words;
    unsigned long long* const d_woff = scratch.word_off;
    char* const d_temp = scratch.temp;
    const size_t scan_bytes = scratch.scan_bytes, sort_bytes = scratch.sort_bytes;
    const uint32_t* const d_start = reads.start;
    const unsigned long long* const d_boff = reads.base_off;
    const uint8_t* const d_ref = reads.ref;

    // ---- words -------------------------------------------------------------------------------------------------------
    HIP_TRY(hipEventRecord(ev[2], stream));
    HIP_TRY(hipMemsetAsync(d_nwords + R, 0, 4, stream));
    HIP_TRY(launch_sam_count(reads, d_keep, d_nwords, stream));
    HIP_TRY(launch_sam_scan(d_nwords, d_woff, R, d_temp, scan_bytes, stream));
    uint32_t bad = 0;
    unsigned long long all_words = 0;
    if (d_bad) HIP_TRY(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&all_words, d_woff + R, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (bad) return set_error(WEPP_EINVAL, "a base byte is not one of 0..5 (ACGTN_)");
    if (all_words > B) return set_error(WEPP_EDEVICE, "more read words than aligned columns");
    uint32_t* d_words;
    DEV_GET(pool, d_words, (size_t)all_words);
    HIP_TRY(launch_sam_words(reads, d_keep, d_woff, d_words, stream));
    HIP_TRY(hipEventRecord(ev[3], stream));

    // ---- order -------------------------------------------------------------------------------------------------------
    uint32_t *d_iota, *d_order, *d_head, *d_goff, *d_lead;
    unsigned long long *d_hoff, *d_moff;
    DEV_GET(pool, d_iota, R); DEV_GET(pool, d_order, R); DEV_GET(pool, d_head, (size_t)R + 1); DEV_GET(pool, d_goff, (size_t)R + 1);
    DEV_GET(pool, d_lead, (size_t)R + 1); DEV_GET(pool, d_hoff, (size_t)R + 1); DEV_GET(pool, d_moff, (size_t)R + 1);
    const SamSortArgs sa{d_start, d_boff, d_woff, d_words, d_ref};
    HIP_TRY(launch_sam_sort(sa, R, d_iota, d_order, d_temp, sort_bytes, stream));
    HIP_TRY(hipEventRecord(ev[4], stream));

    // ---- merge -------------------------------------------------------------------------------------------------------
    HIP_TRY(hipMemsetAsync(d_head + R, 0, 4, stream));
    HIP_TRY(launch_sam_heads(sa, R, d_order, d_head, stream));
    HIP_TRY(launch_sam_scan(d_head, d_hoff, R, d_temp, scan_bytes, stream));
    unsigned long long n_merged64 = 0;
    HIP_TRY(hipMemcpyAsync(&n_merged64, d_hoff + R, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (n_merged64 == 0 || n_merged64 > R) return set_error(WEPP_EDEVICE, "the merge left " + std::to_string(n_merged64) + " reads of " + std::to_string(R));
    const uint32_t M = (uint32_t)n_merged64;
    HIP_TRY(hipMemsetAsync(d_lead + M, 0, 4, stream));
    HIP_TRY(launch_sam_groups(R, d_order, d_head, d_hoff, d_woff, d_goff, d_lead, stream));
    HIP_TRY(launch_sam_scan(d_lead, d_moff, M, d_temp, scan_bytes, stream));
    unsigned long long merged_words = 0;
    HIP_TRY(hipMemcpyAsync(&merged_words, d_moff + M, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (merged_words > all_words) return set_error(WEPP_EDEVICE, "more words in the merged reads than in all reads");
    if (merged_words >= (1ull << 32)) return set_error(WEPP_ELIMIT, "2^32 or more words in the merged reads");
    SamMergedDev md{};
    DEV_GET(pool, md.read_off, (size_t)M + 1); DEV_GET(pool, md.read_word, (size_t)merged_words);
    DEV_GET(pool, md.start, M); DEV_GET(pool, md.end, M); DEV_GET(pool, md.degree, M);
    HIP_TRY(launch_sam_merge(sa, M, d_order, d_goff, d_moff, md, stream));
    HIP_TRY(hipEventRecord(ev[5], stream));

    // ---- outputs -----------------------------------------------------------------------------------------------------
    *out->n_merged = M;
    if (out->freq) HIP_TRY(d2h_staged(out->freq, d_freq, cells * 4, stream));
    HIP_TRY(d2h_staged(out->order, d_order, (size_t)R * 4, stream));
    HIP_TRY(hipMemcpyAsync(out->group_off, d_goff, ((size_t)M + 1) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->read_off, md.read_off, ((size_t)M + 1) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->start, md.start, (size_t)M * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->end, md.end, (size_t)M * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out->degree, md.degree, (size_t)M * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (order_map)
        for (uint32_t s = 0; s < R; s++) out->order[s] = order_map[out->order[s]];
    float ms[4] = {0, 0, 0, 0};
    HIP_TRY(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    for (int i = 1; i < 4; i++) HIP_TRY(hipEventElapsedTime(&ms[i], ev[i + 1], ev[i + 2]));
    g_last.pileup_ms = ms[0]; g_last.correct_ms = ms[1]; g_last.sort_ms = ms[2]; g_last.merge_ms = ms[3];
    if (merged_words > out->word_capacity) {
        // everything else is complete: the words wait for wepp_sam_fetch_words
        try { g_pending.resize((size_t)merged_words); } catch (const std::bad_alloc&) {
            return set_error(WEPP_ENOMEM, "no host memory for the pending read words");
        }
        HIP_TRY(d2h_staged(g_pending.data(), md.read_word, (size_t)merged_words * 4, stream));
        g_have_pending = true;
        return set_error(WEPP_ELIMIT, "read_word holds " + std::to_string(out->word_capacity) + " entries, " + std::to_string(merged_words) +
                                          " needed (read_off is complete: fetch them with wepp_sam_fetch_words)");
    }
    if (merged_words) HIP_TRY(d2h_staged(out->read_word, md.read_word, (size_t)merged_words * 4, stream));
    return WEPP_OK;
}

}  // namespace wepp

extern "C" int wepp_sam_build(int device, const uint8_t* reference, uint32_t genome_size, const wepp_sam_reads* rd,
                              const wepp_sam_params* par, wepp_sam_out* out) {
    if (int rc = sam_check_arguments(reference, genome_size, rd, par, out)) return rc;
    const uint32_t R = rd->n_reads;
    sam_reset_thread_state();
    const size_t cells = (size_t)genome_size * 6;
    if (R == 0) {
        *out->n_merged = 0; out->group_off[0] = 0; out->read_off[0] = 0;
        if (out->freq) std::fill(out->freq, out->freq + cells, 0);
        return WEPP_OK;
    }
    const uint64_t B = rd->base_off[R];
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(WEPP_EDEVICE, "no HIP device found (wepp_place has no CPU fallback)");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = nullptr;

    wepp_mat::DevBlockCache cache;             // (declared before the pool: the pool hands its blocks back first)
    DevPool pool(cache);
    DevEvents<6> ev;
    if (int rc = ev.create()) return rc;

    // ---- the reads and the reference on the device --------------------------------------------------------------
    uint8_t *d_ref, *d_base, *d_keep;
    uint32_t *d_start, *d_freq, *d_bad;
    unsigned long long* d_boff;
    DEV_GET(pool, d_ref, genome_size); DEV_GET(pool, d_base, B); DEV_GET(pool, d_keep, cells); DEV_GET(pool, d_start, R);
    DEV_GET(pool, d_freq, cells); DEV_GET(pool, d_bad, 1); DEV_GET(pool, d_boff, (size_t)R + 1);
    SamScratch scratch;
    if (int rc = sam_get_scratch(pool, R, &scratch)) return rc;
    HIP_TRY(hipMemcpyAsync(d_ref, reference, genome_size, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_start, rd->start, (size_t)R * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_boff, rd->base_off, ((size_t)R + 1) * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_base, rd->base, B, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_freq, 0, cells * 4, stream));
    HIP_TRY(hipMemsetAsync(d_bad, 0, 4, stream));
    SamReadsDev reads{R, d_start, d_boff, d_base, d_ref, genome_size};

    // ---- table, keep table; then the stages both calls share -----------------------------------------------------
    HIP_TRY(hipEventRecord(ev[0], stream));
    HIP_TRY(launch_sam_pileup(reads, d_freq, d_bad, stream));
    HIP_TRY(launch_sam_keep(d_freq, genome_size, par->min_af, par->min_depth, d_keep, stream));
    HIP_TRY(hipEventRecord(ev[1], stream));
    return sam_finish(pool, stream, reads, B, d_keep, d_freq, d_bad, scratch, ev.ev, nullptr, out);
}

