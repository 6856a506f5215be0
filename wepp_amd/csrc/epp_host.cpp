// epp_host.cpp -- the definitions of epp_host.hpp: host code only, shared by the WEPP entry points
#include "epp_host.hpp"
#include <numeric>

namespace wepp {

int epp_validate_reads(const wepp_epp_reads* rd, long long* total_degree_out) {
    const uint32_t R = rd->n_reads;
    long long total_degree = 0;
    for (uint32_t r = 0; r < R; r++) {
        if (rd->read_off[r + 1] < rd->read_off[r]) return set_error(WEPP_EINVAL, "read_off is not monotone");
        if (rd->start[r] < 1 || rd->end[r] < rd->start[r] || (uint32_t)rd->end[r] > WEPP_MAX_POSITION)
            return set_error(WEPP_EINVAL, "read " + std::to_string(r) + ": window must satisfy 1 <= start <= end <= 2^20 - 2");
        if (rd->degree[r] < 0) return set_error(WEPP_EINVAL, "read " + std::to_string(r) + ": negative degree");
        total_degree += rd->degree[r];
        uint32_t prev = 0;
        for (uint32_t j = rd->read_off[r]; j < rd->read_off[r + 1]; j++) {
            const uint32_t w = rd->read_word[j];
            const uint32_t pos = w & 0xFFFFFu, ref = (w >> 20) & 15u, mut = (w >> 24) & 15u;
            if (pos == 0 || pos > WEPP_MAX_POSITION || pos <= prev)
                return set_error(WEPP_EINVAL, "read " + std::to_string(r) + ": mutations must be sorted by position, unique, in 1..2^20-2");
            if (mut == ref || mut == 0)
                return set_error(WEPP_EINVAL, "read " + std::to_string(r) + ": a listed mutation must differ from the reference base (sam2pb.cpp:521-535)");
            prev = pos;
        }
    }
    if (total_degree_out) *total_degree_out = total_degree;
    return WEPP_OK;
}

// order by (start, end, index).  Window bounds are genome positions: two stable counting passes (end,
// then start) instead of a comparison sort through two indirections (≈0.1 s per 1 M reads)
void epp_window_order(const wepp_epp_reads* rd, std::vector<uint32_t>& order) {
    const uint32_t R = rd->n_reads;
    order.resize(R);
    int32_t lo = 0, hi = 0;
    for (uint32_t r = 0; r < R; r++) {
        lo = std::min({lo, rd->start[r], rd->end[r]});
        hi = std::max({hi, rd->start[r], rd->end[r]});
    }
    if (lo < 0 || (uint64_t)hi > (1ull << 24)) {          // not positions: the general way
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            if (rd->start[a] != rd->start[b]) return rd->start[a] < rd->start[b];
            if (rd->end[a] != rd->end[b]) return rd->end[a] < rd->end[b];
            return a < b;
        });
    } else {
        std::vector<uint32_t> tmp(R), cnt((size_t)hi + 2);
        auto pass = [&](const int32_t* key, const uint32_t* in, uint32_t* out) {
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (uint32_t s = 0; s < R; s++) cnt[(size_t)key[in ? in[s] : s] + 1]++;
            for (size_t k = 1; k < cnt.size(); k++) cnt[k] += cnt[k - 1];
            for (uint32_t s = 0; s < R; s++) {
                const uint32_t r = in ? in[s] : s;
                out[cnt[(size_t)key[r]]++] = r;
            }
        };
        pass(rd->end, nullptr, tmp.data());
        pass(rd->start, tmp.data(), order.data());
    }
}

int alloc_reads(DevPool& pool, uint32_t R, uint64_t W, DevReads* d) {
    d->R = R; d->W = W;
    DEV_GET(pool, d->read_off, (size_t)R + 1); DEV_GET(pool, d->read_word, W); DEV_GET(pool, d->order, R);
    DEV_GET(pool, d->start, R); DEV_GET(pool, d->end, R); DEV_GET(pool, d->degree, R);
    return WEPP_OK;
}

int upload_reads(DevPool& pool, const wepp_epp_reads* rd, const std::vector<uint32_t>& order, hipStream_t stream, DevReads* d) {
    const uint32_t R = rd->n_reads;
    if (int rc = alloc_reads(pool, R, rd->read_off[R], d)) return rc;
    HIP_TRY(hipMemcpyAsync(d->read_off, rd->read_off, ((size_t)R + 1) * 4, hipMemcpyHostToDevice, stream));
    if (d->W) HIP_TRY(hipMemcpyAsync(d->read_word, rd->read_word, d->W * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d->order, order.data(), (size_t)R * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d->start, rd->start, (size_t)R * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d->end, rd->end, (size_t)R * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d->degree, rd->degree, (size_t)R * 4, hipMemcpyHostToDevice, stream));
    return WEPP_OK;
}

int check_arena_indices(const char* name, uint32_t n, const uint32_t* idx, uint32_t N) {
    for (uint32_t k = 0; k < n; k++)
        if (idx[k] >= N)
            return set_error(WEPP_EINVAL, std::string(name) + "[" + std::to_string(k) + "] = " + std::to_string(idx[k]) + " is not an arena index of this tree (" + std::to_string(N) + " haplotypes)");
    return WEPP_OK;
}

int check_distinct(uint32_t n, const uint32_t* idx, const char* twice) {
    std::vector<uint32_t> sorted(idx, idx + n);
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t k = 1; k < n; k++)
        if (sorted[k] == sorted[k - 1]) return set_error(WEPP_EINVAL, "haplotype " + std::to_string(sorted[k]) + " is " + twice);
    return WEPP_OK;
}

int assign_check_selection(const wepp_epp_reads* rd, const void* out, uint32_t n_sel, const uint32_t* sel) {
    if (!rd || !out || (n_sel && !sel)) return set_error(WEPP_EINVAL, "null argument");
    if (n_sel == 0) return set_error(WEPP_EINVAL, "empty selection: n_sel must be at least 1");
    return check_distinct(n_sel, sel, "selected more than once");
}

int assign_check_handle(const wepp_mat_t* mat, const wepp_epp_reads* rd, uint32_t n_sel, const uint32_t* sel) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    if (int rc = check_arena_indices("sel", n_sel, sel, mat->dev.N)) return rc;
    if (rd->n_reads && (!rd->read_off || !rd->start || !rd->end || !rd->degree)) return set_error(WEPP_EINVAL, "null read array");
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
    uint32_t *d_sel, *d_bsum, *d_flag;
    uint8_t* d_geno;
    uint16_t* d_pre;
    DEV_GET(pool, d_sel, K); DEV_GET(pool, d_geno, rows * Kp); DEV_GET(pool, d_pre, rows * Kp);
    DEV_GET(pool, d_bsum, (size_t)nblk * Kp); DEV_GET(pool, d_flag, 1);
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
