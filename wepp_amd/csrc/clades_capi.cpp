// clades_capi.cpp -- wepp_mat_set_clades / wepp_clade_assign: host side of the clade assignment of placed samples
// (usher_common.cpp:597-616, written out by :906-967).
//
// The reference calls Tree::get_clade_assignment -- a walk to the root -- once per annotation column and optimal node of
// a sample and sorts the names.  Here the walk is two tables per column built once per handle, the names are ids whose
// order is the names' order, and a batch's (read, optimal node) pairs go through clades_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "clades.hpp"
#include "clades_host.hpp"
#include "epp_host.hpp"
#include "staged_copy.hpp"

namespace {

struct CladeTiming { float pairs_ms = 0, count_ms = 0, finish_ms = 0; };
thread_local CladeTiming g_last;

template <typename T>
int to_device(T* dst, const T* src, size_t n, hipStream_t stream) {
    if (n) HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
    return WEPP_OK;
}

}  // namespace

extern "C" int wepp_clade_last_timing(double* pairs_ms, double* count_ms, double* finish_ms) {
    if (pairs_ms) *pairs_ms = g_last.pairs_ms;
    if (count_ms) *count_ms = g_last.count_ms;
    if (finish_ms) *finish_ms = g_last.finish_ms;
    return WEPP_OK;
}

extern "C" int wepp_mat_set_clades(wepp_mat_t* mat, uint32_t n_columns, const uint32_t* clade_id, const uint32_t* undefined_id) {
    if (!mat) return set_error(WEPP_EINVAL, "null handle");
    if (n_columns > CLADE_MAX_COLUMNS)
        return set_error(WEPP_ELIMIT, std::to_string(n_columns) + " annotation columns, at most " + std::to_string(CLADE_MAX_COLUMNS));
    HIP_TRY(hipSetDevice(mat->device));
    if (n_columns == 0) {
        mat->clade_tab.reset();
        mat->clade_columns = 0;
        return WEPP_OK;
    }
    if (!clade_id || !undefined_id) return set_error(WEPP_EINVAL, "null argument");
    const uint32_t N = mat->dev.N;
    std::vector<uint32_t> parent_dfs(N), tab;
    HIP_TRY(hipMemcpy(parent_dfs.data(), mat->dev.parent_dfs, (size_t)N * 4, hipMemcpyDeviceToHost));
    for (uint32_t d = 1; d < N; d++)
        if (parent_dfs[d] >= d) return set_error(WEPP_EDEVICE, "parent_dfs is not a pre-order");
    clade_build_tables(N, n_columns, parent_dfs.data(), mat->dfs2id.data(), clade_id, undefined_id, tab);
    WEPP_TRY(upload_whole(mat->clade_tab, tab.data(), tab.size(), "clade tables"));
    mat->clade_columns = n_columns;
    return WEPP_OK;
}

extern "C" int wepp_clade_assign(wepp_mat_t* mat, const uint32_t* read_off, const uint32_t* read_word, uint32_t n_reads,
                                 const uint32_t* best_bfs_j, const uint64_t* best_off, const uint32_t* best_nodes,
                                 uint32_t* best_clade, uint64_t* hist_off, uint32_t* hist_clade, uint32_t* hist_count,
                                 uint64_t capacity) {
    if (!mat || !read_off || !best_off || (n_reads && !best_bfs_j)) return set_error(WEPP_EINVAL, "null argument");
    if (mat->clade_columns == 0) return set_error(WEPP_EINVAL, "no clades set on this handle: call wepp_mat_set_clades first");
    const uint32_t R = n_reads, C = mat->clade_columns, N = mat->dev.N;
    if (read_off[0] != 0) return set_error(WEPP_EINVAL, "read_off[0] must be 0");
    for (uint32_t r = 0; r < R; r++)
        if (read_off[r + 1] < read_off[r]) return set_error(WEPP_EINVAL, "read_off not monotone");
    if (read_off[R] && !read_word) return set_error(WEPP_EINVAL, "null read_word");
    if (best_off[0] == 0 && best_off[R] && !best_nodes) return set_error(WEPP_EINVAL, "null best_nodes");
    {
        uint64_t where = 0;
        const int bad = clade_check_pairs(R, N, best_off, best_nodes, &where);
        if (bad == 1) return set_error(WEPP_EINVAL, "best_off[0] must be 0");
        if (bad == 2) return set_error(WEPP_EINVAL, "best_off not monotone at read " + std::to_string(where));
        if (bad == 3) return set_error(WEPP_EINVAL, "best_nodes[" + std::to_string(where) + "] = " + std::to_string(best_nodes[where]) +
                                                        " is not a BFS index of this tree (" + std::to_string(N) + " nodes)");
    }
    const uint64_t P64 = best_off[R];
    if (P64 * C >= (1ull << 32) || ((uint64_t)R + 1) * C >= (1ull << 32))
        return set_error(WEPP_ELIMIT, "columns x pairs (or reads) reach 2^32 in one call; split the batch");
    const uint32_t P = (uint32_t)P64;
    const bool want_hist = hist_off || hist_clade || hist_count;
    g_last = CladeTiming{};
    if (R == 0 || P == 0) {
        // (no read has a node: nothing to assign; a read without nodes cannot hold its best_bfs_j)
        if (R) return set_error(WEPP_EINVAL, "read 0: best_bfs_j is not among the read's nodes");
        if (hist_off) hist_off[0] = 0;
        return WEPP_OK;
    }

    // the reads by the path their segments take (clades.hpp); one pair needs no sort
    std::vector<uint32_t> off32((size_t)R + 1), lists, long_off(1, 0u);
    std::vector<uint32_t> by_wave, by_block, by_long;
    for (uint32_t r = 0; r <= R; r++) off32[r] = (uint32_t)best_off[r];
    if (want_hist)
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t L = off32[r + 1] - off32[r];
            if (L < 2) continue;
            if (L <= CLADE_WAVE_MAX) by_wave.push_back(r);
            else if (L <= CLADE_BLOCK_MAX) by_block.push_back(r);
            else { by_long.push_back(r); long_off.push_back(long_off.back() + L); }
        }
    const uint32_t n_wave = (uint32_t)by_wave.size(), n_block = (uint32_t)by_block.size(), n_long = (uint32_t)by_long.size();
    const uint32_t n_long_pairs = long_off.back();
    lists.reserve((size_t)n_wave + n_block + n_long + long_off.size());
    lists.insert(lists.end(), by_wave.begin(), by_wave.end());
    lists.insert(lists.end(), by_block.begin(), by_block.end());
    lists.insert(lists.end(), by_long.begin(), by_long.end());
    lists.insert(lists.end(), long_off.begin(), long_off.end());

    HIP_TRY(hipSetDevice(mat->device));
    hipStream_t stream = nullptr;
    DevPool pool(mat->epp_cache);
    const uint64_t nw = read_off[R], CP = (uint64_t)C * P;
    uint32_t *d_roff, *d_rword, *d_bj, *d_boff, *d_bnodes, *d_lists;
    uint32_t *d_pread, *d_keys, *d_sorted, *d_bclade, *d_found;
    DEV_GET(pool, d_roff, (size_t)R + 1); DEV_GET(pool, d_rword, std::max<uint64_t>(nw, 1)); DEV_GET(pool, d_bj, R);
    DEV_GET(pool, d_boff, (size_t)R + 1); DEV_GET(pool, d_bnodes, P); DEV_GET(pool, d_lists, lists.size());
    DEV_GET(pool, d_pread, P); DEV_GET(pool, d_keys, CP); DEV_GET(pool, d_sorted, CP);
    DEV_GET(pool, d_bclade, (size_t)C * R); DEV_GET(pool, d_found, R);
    uint32_t *d_head = nullptr, *d_runof = nullptr;
    unsigned long long *d_hoff = nullptr, *d_k64a = nullptr, *d_k64b = nullptr;
    char *d_scan_tmp = nullptr, *d_sort_tmp = nullptr;
    size_t scan_bytes = 0, sort_bytes = 0;
    uint32_t end_bit = 32;
    if (want_hist) {
        DEV_GET(pool, d_head, CP + 1); DEV_GET(pool, d_runof, CP + 1); DEV_GET(pool, d_hoff, (size_t)C * R + 1);
        HIP_TRY(clade_scan_temp_bytes(CP + 1, &scan_bytes));
        DEV_GET(pool, d_scan_tmp, std::max<size_t>(scan_bytes, 1));
        if (n_long) {
            const uint64_t n_keys = (uint64_t)C * n_long_pairs;
            while (end_bit < 64 && ((uint64_t)C * n_long) >> (end_bit - 32)) end_bit++;
            DEV_GET(pool, d_k64a, n_keys); DEV_GET(pool, d_k64b, n_keys);
            HIP_TRY(clade_sort_long_temp_bytes(n_keys, end_bit, &sort_bytes));
            DEV_GET(pool, d_sort_tmp, std::max<size_t>(sort_bytes, 1));
        }
    }
    DevEvents<4> ev;
    if (int rc = ev.create()) return rc;

    if (int rc = to_device(d_roff, read_off, (size_t)R + 1, stream)) return rc;
    if (int rc = to_device(d_rword, read_word, nw, stream)) return rc;
    if (int rc = to_device(d_bj, best_bfs_j, R, stream)) return rc;
    if (int rc = to_device(d_boff, off32.data(), (size_t)R + 1, stream)) return rc;
    if (int rc = to_device(d_bnodes, best_nodes, P, stream)) return rc;
    if (int rc = to_device(d_lists, lists.data(), lists.size(), stream)) return rc;
    HIP_TRY(hipMemsetAsync(d_found, 0, (size_t)R * 4, stream));

    CladeArgs a{};
    a.R = R; a.C = C; a.P = P;
    a.read_off = d_roff; a.read_word = d_rword; a.best_bfs_j = d_bj; a.best_off = d_boff; a.best_nodes = d_bnodes;
    a.tab = mat->clade_tab.ptr;
    a.pair_read = d_pread; a.keys = d_keys; a.sorted = d_sorted; a.best_clade = d_bclade; a.found = d_found;

    // ---- the pairs ------------------------------------------------------------------------------------
    HIP_TRY(hipEventRecord(ev[0], stream));
    HIP_TRY(launch_clade_pairs(mat->dev, a, stream));
    HIP_TRY(hipEventRecord(ev[1], stream));

    // ---- every segment sorted, run heads, their scan ---------------------------------------------------
    if (want_hist) {
        const uint32_t *l_wave = d_lists, *l_block = l_wave + n_wave, *l_long = l_block + n_block, *l_loff = l_long + n_long;
        HIP_TRY(launch_clade_sort_wave(a, l_wave, n_wave, stream));
        HIP_TRY(launch_clade_sort_block(a, l_block, n_block, stream));
        HIP_TRY(launch_clade_sort_long(a, l_long, l_loff, n_long, n_long_pairs, d_k64a, d_k64b, end_bit, d_sort_tmp, sort_bytes, stream));
        HIP_TRY(launch_clade_heads(a, d_head, d_runof, d_hoff, d_scan_tmp, scan_bytes, stream));
    }
    HIP_TRY(hipEventRecord(ev[2], stream));

    // ---- what can be said before the runs are written ---------------------------------------------------
    std::vector<uint32_t> found(R);
    uint32_t n_runs = 0;
    HIP_TRY(hipMemcpyAsync(found.data(), d_found, (size_t)R * 4, hipMemcpyDeviceToHost, stream));
    if (want_hist) HIP_TRY(hipMemcpyAsync(&n_runs, d_runof + CP, 4, hipMemcpyDeviceToHost, stream));
    {
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_fail(e, "clade kernels");
    }
    for (uint32_t r = 0; r < R; r++)
        if (!found[r])
            return set_error(WEPP_EINVAL, "read " + std::to_string(r) + ": best_bfs_j = " + std::to_string(best_bfs_j[r]) +
                                              " is not among the read's nodes");
    if (best_clade) HIP_TRY(d2h_staged(best_clade, d_bclade, (size_t)C * R * 4, stream));
    if (hist_off) HIP_TRY(d2h_staged(hist_off, d_hoff, ((size_t)C * R + 1) * 8, stream));
    const bool want_runs = hist_clade || hist_count;
    const bool short_runs = want_runs && n_runs > capacity;
    if (want_runs && !short_runs && n_runs) {
        uint32_t *d_rstart, *d_hclade = nullptr, *d_hcount = nullptr;
        DEV_GET(pool, d_rstart, (size_t)n_runs + 1);
        if (hist_clade) DEV_GET(pool, d_hclade, n_runs);
        if (hist_count) DEV_GET(pool, d_hcount, n_runs);
        HIP_TRY(launch_clade_runs(a, d_head, d_runof, n_runs, d_rstart, d_hclade, d_hcount, stream));
        if (hist_clade) HIP_TRY(d2h_staged(hist_clade, d_hclade, (size_t)n_runs * 4, stream));
        if (hist_count) HIP_TRY(d2h_staged(hist_count, d_hcount, (size_t)n_runs * 4, stream));
    }
    HIP_TRY(hipEventRecord(ev[3], stream));
    HIP_TRY(hipStreamSynchronize(stream));
    (void)hipEventElapsedTime(&g_last.pairs_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&g_last.count_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&g_last.finish_ms, ev[2], ev[3]);
    if (short_runs)
        return set_error(WEPP_ELIMIT, "hist_clade / hist_count hold " + std::to_string(capacity) + " entries, " + std::to_string(n_runs) +
                                          " needed: best_clade and hist_off are complete, call again with buffers of hist_off[n_columns * n_reads] entries");
    return WEPP_OK;
}
