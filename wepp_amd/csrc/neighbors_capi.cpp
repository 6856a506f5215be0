// neighbors_capi.cpp -- wepp_epp_neighbors / wepp_epp_distances: host side of the neighbour sets
// (arena::closest_neighbors, arena::highest_scoring_neighbors, src/WEPP/arena.cpp:171-249).
//
// The reference probes every node it visits with a merge of two stack_muts lists.  Here the pivots' genotypes
// become the position-major table of wepp_epp_assign, the distances of all nodes to all pivots of a pass come out
// of one scatter and one column scan, and the regions out of a second scan (neighbors_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "epp_host.hpp"
#include "neighbors.hpp"
#include "staged_copy.hpp"

namespace {

struct NeighborsTiming { float tables_ms = 0, field_ms = 0, region_ms = 0; };
thread_local NeighborsTiming g_last;

int check_pivots(const wepp_mat_t* mat, uint32_t n_piv, const uint32_t* piv, int form) {
    if (!mat || !piv) return set_error(WEPP_EINVAL, "null argument");
    if (n_piv == 0) return set_error(WEPP_EINVAL, "no pivots: n_piv must be at least 1");
    if (form != WEPP_NBR_TO_PIVOT && form != WEPP_NBR_FROM_PIVOT)
        return set_error(WEPP_EINVAL, "unknown form " + std::to_string(form) + ": WEPP_NBR_TO_PIVOT or WEPP_NBR_FROM_PIVOT");
    if (int rc = check_arena_indices("piv", n_piv, piv, mat->dev.N)) return rc;
    return check_distinct(n_piv, piv, "a pivot more than once");
}

// the handle's dfs_end (device) and its forced pass size, made by the first call
int prepare_handle(wepp_mat_t* mat) {
    if (mat->nbr_pass_cols < 0) {
        const char* s = std::getenv("WEPP_NBR_PASS_COLS");
        const long v = s ? std::strtol(s, nullptr, 10) : 0;
        mat->nbr_pass_cols = v > 0 ? (int)std::min<long>(v, 1 << 20) : 0;
    }
    if (mat->nbr_dfs_end) return WEPP_OK;
    const uint32_t N = mat->dev.N;
    std::vector<uint32_t> parent(N), end(N);
    HIP_TRY(hipMemcpy(parent.data(), mat->dev.parent_dfs, (size_t)N * 4, hipMemcpyDeviceToHost));
    // reverse pre-order visits children before parents
    for (uint32_t d = 0; d < N; d++) end[d] = d + 1;
    for (uint32_t d = N; d-- > 1;) end[parent[d]] = std::max(end[parent[d]], end[d]);
    // (the handle takes the block once it is filled: a call that fails here leaves none, and the next one tries again)
    WEPP_TRY(upload_whole(mat->nbr_dfs_end, end.data(), N, "dfs_end"));
    mat->stats.device_bytes += std::max<size_t>((size_t)N * 4, 16);
    return WEPP_OK;
}

// Both entry points.  out != nullptr: the regions; dist != nullptr: the field.
int run(wepp_mat_t* mat, uint32_t K, const uint32_t* piv, uint32_t radius, int form, const uint8_t* skip, wepp_neighbors_out* out,
        int32_t* dist) {
    HIP_TRY(hipSetDevice(mat->device));
    if (int rc = prepare_handle(mat)) return rc;
    const uint32_t N = mat->dev.N;
    const uint64_t rows = (uint64_t)N + 1;
    // columns per pass: the two row tables within NBR_PASS_BYTES, the genotype table within wepp_epp_assign's limit
    uint64_t cols = NBR_PASS_BYTES / (rows * 8) / NBR_LANE_COLS * NBR_LANE_COLS;
    if (cols == 0)
        return set_error(WEPP_ELIMIT, "a tree of " + std::to_string(N) + " haplotypes needs more than 2 GiB of device tables for 4 pivots");
    const uint64_t table_cols = ASG_MAX_TABLE_BYTES / (((uint64_t)mat->dev.max_pos + 1) * 3) / ASG_SLAB * ASG_SLAB;
    if (table_cols) cols = std::min(cols, table_cols);        // (none fit: assign_build_table says so)
    if (mat->nbr_pass_cols > 0) cols = (uint64_t)mat->nbr_pass_cols;
    const uint32_t pass_cols = (uint32_t)std::min<uint64_t>(cols, K);
    const uint32_t Es_max = nbr_stride(pass_cols);
    const uint32_t nblk = nbr_scan_blocks((uint32_t)rows);

    hipStream_t stream = nullptr;
    DevPool pool(mat->epp_cache);
    int32_t *d_field, *d_over = nullptr, *d_tover = nullptr;
    uint32_t *d_piv, *d_bsum, *d_bcnt = nullptr, *d_top = nullptr, *d_tend = nullptr, *d_nreg = nullptr, *d_nlist = nullptr;
    uint8_t* d_skip = nullptr;
    unsigned long long* d_off = nullptr;
    char* d_temp = nullptr;
    size_t temp_bytes = 0;
    DEV_GET(pool, d_piv, K); DEV_GET(pool, d_field, rows * Es_max); DEV_GET(pool, d_bsum, (size_t)nblk * Es_max);
    if (out) {
        DEV_GET(pool, d_over, rows * Es_max); DEV_GET(pool, d_bcnt, (size_t)nblk * Es_max); DEV_GET(pool, d_top, Es_max); DEV_GET(pool, d_tend, Es_max);
        DEV_GET(pool, d_tover, Es_max); DEV_GET(pool, d_nreg, Es_max); DEV_GET(pool, d_nlist, (size_t)Es_max + 1); DEV_GET(pool, d_off, (size_t)Es_max + 1);
        HIP_TRY(assign_scan_temp_bytes(Es_max, &temp_bytes));
        DEV_GET(pool, d_temp, temp_bytes);
        if (skip) {
            DEV_GET(pool, d_skip, N);
            HIP_TRY(hipMemcpyAsync(d_skip, skip, N, hipMemcpyHostToDevice, stream));
        }
    }
    HIP_TRY(hipMemcpyAsync(d_piv, piv, (size_t)K * 4, hipMemcpyHostToDevice, stream));

    DevEvents<5> ev;
    if (int rc = ev.create()) return rc;

    NbrTree t{};
    t.N = N; t.max_pos = mat->dev.max_pos;
    t.node_woff = mat->dev.node_woff; t.words = mat->dev.words; t.parent_dfs = mat->dev.parent_dfs; t.dfs_end = mat->nbr_dfs_end;

    g_last = NeighborsTiming{};
    std::vector<unsigned long long> off;
    std::vector<int32_t> h_field;
    uint64_t base = 0;          // entries of the lists of the passes so far
    bool short_lists = false;
    for (uint32_t k0 = 0; k0 < K; k0 += pass_cols) {
        const uint32_t Kc = std::min(pass_cols, K - k0), Es = nbr_stride(Kc);
        DevPool pass_pool(mat->epp_cache);        // the pass's genotype table and lists: back in the cache for the next pass
        AssignTable tab;
        if (int rc = assign_build_table(mat, pass_pool, Kc, piv + k0, stream, ev[0], ev[1], &tab)) return rc;

        // ---- the distance field ------------------------------------------------------------------------
        HIP_TRY(hipMemsetAsync(d_field, 0, rows * Es * 4, stream));
        HIP_TRY(launch_nbr_deltas(t, tab.geno, tab.Kp, Es, form, d_field, stream));
        HIP_TRY(launch_nbr_colscan(d_field, Es, N, d_bsum, stream));
        HIP_TRY(hipEventRecord(ev[2], stream));
        float ms = 0;
        if (dist) {
            h_field.resize((size_t)N * Es);
            HIP_TRY(d2h_staged(h_field.data(), d_field, (size_t)N * Es * 4, stream));
            for (uint32_t j = 0; j < Kc; j++) {
                int32_t* row = dist + (size_t)(k0 + j) * N;
                for (uint32_t n = 0; n < N; n++) row[n] = h_field[(size_t)n * Es + j];
            }
        } else {
            // ---- the regions ---------------------------------------------------------------------------
            HIP_TRY(hipMemsetAsync(d_over, 0, rows * Es * 4, stream));
            HIP_TRY(hipMemsetAsync(d_nreg, 0, (size_t)Es * 4, stream));
            HIP_TRY(hipMemsetAsync(d_nlist, 0, ((size_t)Es + 1) * 4, stream));     // (element Kc: the scan's total)
            HIP_TRY(launch_nbr_over(t, d_field, Es, radius, d_over, stream));
            HIP_TRY(launch_nbr_colscan(d_over, Es, N, d_bsum, stream));
            HIP_TRY(launch_nbr_tops(t, d_piv + k0, Kc, d_field, d_over, Es, radius, d_top, d_tend, d_tover, stream));
            HIP_TRY(launch_nbr_count(N, d_over, Es, d_top, d_tend, d_tover, d_skip, d_bcnt, d_nreg, d_nlist, stream));
            HIP_TRY(launch_assign_scan(d_nlist, d_off, Kc, d_temp, temp_bytes, stream));
            off.resize((size_t)Kc + 1);
            HIP_TRY(hipMemcpyAsync(off.data(), d_off, ((size_t)Kc + 1) * 8, hipMemcpyDeviceToHost, stream));
            if (out->top) HIP_TRY(hipMemcpyAsync(out->top + k0, d_top, (size_t)Kc * 4, hipMemcpyDeviceToHost, stream));
            if (out->n_region) HIP_TRY(hipMemcpyAsync(out->n_region + k0, d_nreg, (size_t)Kc * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            for (uint32_t j = 0; j < Kc; j++) out->nbr_off[k0 + j] = base + off[j];
            const uint64_t need = off[Kc];
            // too small a buffer leaves the lists out from here on, everything else stands
            if (base + need > out->nbr_capacity) short_lists = true;
            uint32_t* d_node = nullptr;
            int32_t* d_dist = nullptr;
            if (need && !short_lists) {
                DEV_GET(pass_pool, d_node, need); DEV_GET(pass_pool, d_dist, need);
                HIP_TRY(launch_nbr_write(N, Kc, d_field, d_over, Es, d_top, d_tend, d_tover, d_skip, d_bcnt, d_off, d_node, d_dist, stream));
            }
            HIP_TRY(hipEventRecord(ev[3], stream));
            if (d_node) {
                HIP_TRY(d2h_staged(out->nbr_node + base, d_node, need * 4, stream));
                HIP_TRY(d2h_staged(out->nbr_dist + base, d_dist, need * 4, stream));
            }
            base += need;
            HIP_TRY(hipStreamSynchronize(stream));
            if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) g_last.region_ms += ms;
        }
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) g_last.tables_ms += ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) g_last.field_ms += ms;
    }
    if (out) {
        out->nbr_off[K] = base;
        if (short_lists)
            return set_error(WEPP_ELIMIT, "nbr_node / nbr_dist hold " + std::to_string(out->nbr_capacity) + " entries, " + std::to_string(base) +
                                              " needed: every other output is complete, call again with buffers of nbr_off[n_piv] entries");
    }
    return WEPP_OK;
}

}  // namespace

int wepp::nbr_prepare_handle(wepp_mat_t* mat) { return prepare_handle(mat); }   // (wepp_epp_peaks runs the field kernels itself)

extern "C" int wepp_epp_neighbors_last_timing(double* tables_ms, double* field_ms, double* region_ms) {
    if (tables_ms) *tables_ms = g_last.tables_ms;
    if (field_ms) *field_ms = g_last.field_ms;
    if (region_ms) *region_ms = g_last.region_ms;
    return WEPP_OK;
}

extern "C" int wepp_epp_neighbors(wepp_mat_t* mat, uint32_t n_piv, const uint32_t* piv, uint32_t radius, int form, const uint8_t* skip,
                                  wepp_neighbors_out* out) {
    if (!out || !out->nbr_off) return set_error(WEPP_EINVAL, "null argument");
    if (int rc = check_pivots(mat, n_piv, piv, form)) return rc;
    if (out->nbr_capacity && (!out->nbr_node || !out->nbr_dist)) return set_error(WEPP_EINVAL, "null output array: nbr_node and nbr_dist hold nbr_capacity entries");
    return run(mat, n_piv, piv, radius, form, skip, out, nullptr);
}

extern "C" int wepp_epp_distances(wepp_mat_t* mat, uint32_t n_piv, const uint32_t* piv, int form, int32_t* dist) {
    if (!dist) return set_error(WEPP_EINVAL, "null argument");
    if (int rc = check_pivots(mat, n_piv, piv, form)) return rc;
    if ((uint64_t)n_piv * mat->dev.N > NBR_MAX_FIELD_CELLS)
        return set_error(WEPP_ELIMIT, "the distance field of " + std::to_string(n_piv) + " pivots over " + std::to_string(mat->dev.N) +
                                          " haplotypes has more than 2^28 cells: ask for the pivots in parts");
    return run(mat, n_piv, piv, 0, form, nullptr, nullptr, dist);
}
