// geno_capi.cpp -- wepp_geno_diameters and wepp_geno_nearest: host side of the pairwise genotype distances behind
// dump_haplotype_uncertainty (src/WEPP/arena.cpp:494-528) and print_mutation_distance (:251-301).
//
// words -> (set, position) keys -> radix sort -> heads -> scan -> columns per set and per word (once per call), then
// per pass: zeroed planes <- the words' bits, small groups by waves, larger groups (and A x B) by tiles.  The calls
// take no tree handle: their device blocks come from a cache of their own that lives as long as the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "epp_host.hpp"
#include "geno.hpp"

namespace {

typedef unsigned long long u64;

struct GenoTiming { double columns_ms = 0, planes_ms = 0, pairs_ms = 0; };
thread_local GenoTiming g_last;

// the checks of a wepp_genotypes both entry points make
int check_genotypes(const wepp_genotypes* g) {
    if (!g || !g->item_off) return set_error(WEPP_EINVAL, "null argument");
    const uint32_t n = g->n_items;
    if (n >= (1u << 31)) return set_error(WEPP_ELIMIT, "2^31 or more items in one call");
    if (g->item_off[0] != 0) return set_error(WEPP_EINVAL, "item_off[0] is not 0");
    for (uint32_t i = 0; i < n; i++)
        if (g->item_off[i + 1] < g->item_off[i]) return set_error(WEPP_EINVAL, "item_off does not ascend at item " + std::to_string(i));
    if (g->item_off[n] >= (1ull << 32)) return set_error(WEPP_ELIMIT, "2^32 or more words in one call");
    if (g->item_off[n] && !g->item_word) return set_error(WEPP_EINVAL, "null argument");
    for (uint32_t i = 0; i < n; i++) {
        int64_t prev = -1;
        for (uint64_t k = g->item_off[i]; k < g->item_off[i + 1]; k++) {
            const uint32_t w = g->item_word[k], pos = w & 0xFFFFFu, ref = (w >> 20) & 15, mut = (w >> 24) & 15;
            auto bad = [&](const char* what) {
                return set_error(WEPP_EINVAL, "item " + std::to_string(i) + ", word " + std::to_string(k - g->item_off[i]) + ": " + what);
            };
            if (w >> 28) return bad("bits above mut_nuc are set");
            if (pos > WEPP_MAX_POSITION) return bad("position exceeds WEPP_MAX_POSITION");
            if ((int64_t)pos <= prev) return bad("positions are not strictly ascending");
            if (mut == 0) return bad("mut_nuc is 0");
            if (mut == ref) return bad("mut_nuc equals ref_nuc");
            prev = pos;
        }
    }
    return WEPP_OK;
}

uint32_t bit_length(uint32_t v) { uint32_t b = 0; while (v) { b++; v >>= 1; } return b; }

struct Columns {                       // what the column phase leaves: per word its column, per set its column count
    GenoWords words{};
    uint32_t* word_col = nullptr;
    std::vector<uint32_t> set_cols;
};

// Uploads the words, the offsets and the keep mask and runs the column phase over n_sets sets (set_off on the host, or
// null for one set); waits for it.
int build_columns(DevPool& pool, const wepp_genotypes* g, uint32_t n_sets, const uint32_t* set_off, const uint32_t* keep_bits,
                  uint32_t keep_positions, hipStream_t stream, Columns* c) {
    const uint32_t n = g->n_items;
    const u64 nw = g->item_off[n];
    u64* d_item_off; uint32_t *d_words, *d_set_off = nullptr, *d_keep = nullptr;
    DEV_GET(pool, d_item_off, (size_t)n + 1); DEV_GET(pool, d_words, (size_t)nw);
    HIP_TRY(hipMemcpyAsync(d_item_off, g->item_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, stream));
    if (nw) HIP_TRY(hipMemcpyAsync(d_words, g->item_word, (size_t)nw * 4, hipMemcpyHostToDevice, stream));
    if (set_off) {
        DEV_GET(pool, d_set_off, (size_t)n_sets + 1);
        HIP_TRY(hipMemcpyAsync(d_set_off, set_off, ((size_t)n_sets + 1) * 4, hipMemcpyHostToDevice, stream));
    }
    if (keep_bits) {
        const size_t kw = ((size_t)keep_positions + 31) / 32;
        DEV_GET(pool, d_keep, kw);
        if (kw) HIP_TRY(hipMemcpyAsync(d_keep, keep_bits, kw * 4, hipMemcpyHostToDevice, stream));
    }
    c->words = GenoWords{nw, n, n_sets, d_item_off, d_words, d_set_off, d_keep, keep_positions};
    c->set_cols.assign(n_sets, 0);
    DEV_GET(pool, c->word_col, (size_t)nw);
    if (nw == 0) return WEPP_OK;

    const uint32_t key_bits = GENO_POS_BITS + bit_length(n_sets);
    u64 *d_key, *d_key2; uint32_t *d_val, *d_val2, *d_head, *d_rank, *d_first, *d_cols;
    DEV_GET(pool, d_key, (size_t)nw); DEV_GET(pool, d_key2, (size_t)nw); DEV_GET(pool, d_val, (size_t)nw); DEV_GET(pool, d_val2, (size_t)nw);
    DEV_GET(pool, d_head, (size_t)nw + 1); DEV_GET(pool, d_rank, (size_t)nw + 1); DEV_GET(pool, d_first, n_sets); DEV_GET(pool, d_cols, n_sets);
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(geno_sort_temp_bytes(nw, key_bits, &sort_bytes));
    HIP_TRY(geno_scan_temp_bytes(nw, &scan_bytes));
    char* d_temp;
    DEV_GET(pool, d_temp, std::max(sort_bytes, scan_bytes));
    HIP_TRY(hipMemsetAsync(d_cols, 0, (size_t)n_sets * 4, stream));
    HIP_TRY(launch_geno_keys(c->words, d_key, d_val, stream));
    HIP_TRY(launch_geno_sort(d_key, d_key2, d_val, d_val2, nw, key_bits, d_temp, sort_bytes, stream));
    HIP_TRY(launch_geno_heads(d_key2, nw, n_sets, d_head, stream));
    HIP_TRY(launch_geno_scan(d_head, d_rank, nw, d_temp, scan_bytes, stream));
    HIP_TRY(launch_geno_sets(d_key2, d_head, d_rank, nw, n_sets, d_first, d_cols, stream));
    HIP_TRY(launch_geno_word_cols(d_key2, d_val2, d_head, d_rank, nw, n_sets, d_first, c->word_col, stream));
    HIP_TRY(hipMemcpyAsync(c->set_cols.data(), d_cols, (size_t)n_sets * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return WEPP_OK;
}

struct PassTables {                    // a pass's tables on the host and on the device
    std::vector<u64> base;
    std::vector<uint32_t> item0, items, words;
    u64 plane_words = 0;
    GenoPass dev{};
};

// the sets [s0, s1) as a pass: tables, zeroed planes, the planes filled.  Sets of fewer than min_items items get no
// planes (W = 0: k_geno_planes passes over their words).
int build_planes(DevPool& pool, const Columns& c, const wepp_genotypes* g, uint32_t s0, uint32_t s1, const uint32_t* set_off, uint32_t min_items,
                 hipStream_t stream, PassTables* t) {
    const uint32_t ns = s1 - s0;
    t->base.resize(ns); t->item0.resize(ns); t->items.resize(ns); t->words.resize(ns);
    t->plane_words = 0;
    for (uint32_t s = s0; s < s1; s++) {
        const uint32_t k = s - s0, i0 = set_off ? set_off[s] : 0, i1 = set_off ? set_off[s + 1] : g->n_items;
        t->base[k] = t->plane_words; t->item0[k] = i0; t->items[k] = i1 - i0; t->words[k] = i1 - i0 >= min_items ? (c.set_cols[s] + 63) / 64 : 0;
        t->plane_words += (u64)(i1 - i0) * t->words[k] * 4;
    }
    u64 *d_base, *d_planes; uint32_t *d_item0, *d_items, *d_words;
    DEV_GET(pool, d_base, ns); DEV_GET(pool, d_item0, ns); DEV_GET(pool, d_items, ns); DEV_GET(pool, d_words, ns);
    DEV_GET(pool, d_planes, (size_t)t->plane_words);
    HIP_TRY(hipMemcpyAsync(d_base, t->base.data(), (size_t)ns * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_item0, t->item0.data(), (size_t)ns * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_items, t->items.data(), (size_t)ns * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_words, t->words.data(), (size_t)ns * 4, hipMemcpyHostToDevice, stream));
    if (t->plane_words) HIP_TRY(hipMemsetAsync(d_planes, 0, (size_t)t->plane_words * 8, stream));
    const uint32_t i0 = t->item0[0], i1 = t->item0[ns - 1] + t->items[ns - 1];
    t->dev = GenoPass{s0, ns, i0, i1 - i0, d_base, d_item0, d_items, d_words, d_planes};
    if (t->plane_words) HIP_TRY(launch_geno_planes(c.words, c.word_col, t->dev, g->item_off[i0], g->item_off[i1], stream));
    return WEPP_OK;
}

// the plane bytes of set s
u64 set_bytes(const Columns& c, const uint32_t* set_off, uint32_t s) {
    return (u64)(set_off[s + 1] - set_off[s]) * ((c.set_cols[s] + 63) / 64) * 32;
}

int open_device(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return set_error(WEPP_EDEVICE, "no HIP device found (wepp_place has no CPU fallback)");
    HIP_TRY(hipSetDevice(device));
    return WEPP_OK;
}

// runs the listed tiles in launches of at most GENO_JOBS_PER_LAUNCH; next(job) fills the next tile or returns false
template <typename Next, typename Launch>
int run_tiles(DevPool& pool, hipStream_t stream, Next next, Launch launch) {
    std::vector<GenoTileJob> jobs;
    GenoTileJob* d_jobs = nullptr;
    for (bool more = true; more;) {
        jobs.clear();
        GenoTileJob j;
        while (jobs.size() < GENO_JOBS_PER_LAUNCH && (more = next(&j))) jobs.push_back(j);
        if (jobs.empty()) break;
        if (!d_jobs) DEV_GET(pool, d_jobs, jobs.size());   // (the first list is the longest)
        HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(GenoTileJob), hipMemcpyHostToDevice, stream));
        HIP_TRY(launch((const GenoTileJob*)d_jobs, (uint32_t)jobs.size()));
        HIP_TRY(hipStreamSynchronize(stream));   // (the host list is reused)
    }
    return WEPP_OK;
}

}  // namespace

extern "C" int wepp_geno_last_timing(double* columns_ms, double* planes_ms, double* pairs_ms) {
    if (columns_ms) *columns_ms = g_last.columns_ms;
    if (planes_ms) *planes_ms = g_last.planes_ms;
    if (pairs_ms) *pairs_ms = g_last.pairs_ms;
    return WEPP_OK;
}

extern "C" int wepp_geno_diameters(int device, const wepp_genotypes* g, const uint32_t* keep_bits, uint32_t keep_positions, uint32_t n_groups,
                                   const uint32_t* grp_off, int32_t* diam) {
    if (!g || !grp_off || (n_groups && !diam)) return set_error(WEPP_EINVAL, "null argument");
    if (int rc = check_genotypes(g)) return rc;
    if (grp_off[0] != 0) return set_error(WEPP_EINVAL, "grp_off[0] is not 0");
    for (uint32_t s = 0; s < n_groups; s++)
        if (grp_off[s + 1] < grp_off[s]) return set_error(WEPP_EINVAL, "grp_off does not ascend at group " + std::to_string(s));
    if (grp_off[n_groups] != g->n_items)
        return set_error(WEPP_EINVAL, "grp_off ends at " + std::to_string(grp_off[n_groups]) + ", not at n_items = " + std::to_string(g->n_items));
    g_last = GenoTiming{};
    if (n_groups == 0) return WEPP_OK;
    // the pass bound: read once per call; it only ever lowers GENO_PASS_BYTES
    u64 pass_bytes = GENO_PASS_BYTES;
    if (const char* s = std::getenv("WEPP_GENO_PASS_BYTES")) {
        const u64 v = std::strtoull(s, nullptr, 10);
        if (v > 0) pass_bytes = std::min<u64>(v, GENO_PASS_BYTES);
    }
    if (int rc = open_device(device)) return rc;
    hipStream_t stream = nullptr;
    wepp_mat::DevBlockCache cache;             // (declared before the pools: they hand their blocks back first)
    DevPool pool(cache);
    DevEvents<4> ev;
    if (int rc = ev.create()) return rc;

    Columns c;
    HIP_TRY(hipEventRecord(ev[0], stream));
    if (int rc = build_columns(pool, g, n_groups, grp_off, keep_bits, keep_positions, stream, &c)) return rc;
    HIP_TRY(hipEventRecord(ev[1], stream));
    for (uint32_t s = 0; s < n_groups; s++)
        if (set_bytes(c, grp_off, s) > GENO_PASS_BYTES)
            return set_error(WEPP_ELIMIT, "group " + std::to_string(s) + " (" + std::to_string(grp_off[s + 1] - grp_off[s]) + " items, " +
                                              std::to_string(c.set_cols[s]) + " columns) needs " + std::to_string(set_bytes(c, grp_off, s)) +
                                              " bytes of planes, more than a pass holds (" + std::to_string(GENO_PASS_BYTES) + ")");
    int32_t* d_diam;
    DEV_GET(pool, d_diam, n_groups);
    HIP_TRY(hipMemsetAsync(d_diam, 0, (size_t)n_groups * 4, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    g_last.columns_ms = ms;

    for (uint32_t s0 = 0; s0 < n_groups;) {
        // groups of fewer than two items have diameter 0 and no planes; a pass takes groups while they fit (at least one)
        u64 bytes = 0;
        uint32_t s1 = s0;
        while (s1 < n_groups) {
            const u64 b = grp_off[s1 + 1] - grp_off[s1] >= 2 ? set_bytes(c, grp_off, s1) : 0;
            if (s1 > s0 && bytes + b > pass_bytes) break;
            bytes += b; s1++;
        }
        {
            DevPool pass_pool(cache);          // the pass's blocks go back to the cache at its end
            PassTables t;
            HIP_TRY(hipEventRecord(ev[1], stream));
            if (int rc = build_planes(pass_pool, c, g, s0, s1, grp_off, 2, stream, &t)) return rc;
            HIP_TRY(hipEventRecord(ev[2], stream));
            std::vector<uint32_t> small;
            for (uint32_t k = 0; k < s1 - s0; k++)
                if (t.items[k] >= 2 && t.items[k] <= GENO_WAVE_ITEMS) small.push_back(k);
            if (!small.empty()) {
                uint32_t* d_small;
                DEV_GET(pass_pool, d_small, small.size());
                HIP_TRY(hipMemcpyAsync(d_small, small.data(), small.size() * 4, hipMemcpyHostToDevice, stream));
                HIP_TRY(launch_geno_wave(t.dev, d_small, (uint32_t)small.size(), d_diam, stream));
            }
            uint32_t k = 0, ti = 0, tj = 0;    // the next tile: the upper triangle of every larger group, row by row
            auto next = [&](GenoTileJob* j) {
                for (; k < s1 - s0; k++, ti = 0, tj = 0) {
                    if (t.items[k] <= GENO_WAVE_ITEMS) continue;
                    const uint32_t T = (t.items[k] + GENO_TILE - 1) / GENO_TILE;
                    if (ti >= T) continue;
                    *j = GenoTileJob{k, ti, tj};
                    if (++tj == T) { ti++; tj = ti; }
                    return true;
                }
                return false;
            };
            if (int rc = run_tiles(pass_pool, stream, next, [&](const GenoTileJob* d_jobs, uint32_t n) { return launch_geno_tile_diam(t.dev, d_jobs, n, d_diam, stream); }))
                return rc;
            HIP_TRY(hipEventRecord(ev[3], stream));
            HIP_TRY(hipStreamSynchronize(stream));
            float pm = 0, qm = 0;
            HIP_TRY(hipEventElapsedTime(&pm, ev[1], ev[2]));
            HIP_TRY(hipEventElapsedTime(&qm, ev[2], ev[3]));
            g_last.planes_ms += pm; g_last.pairs_ms += qm;
        }
        s0 = s1;
    }
    HIP_TRY(hipMemcpyAsync(diam, d_diam, (size_t)n_groups * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return WEPP_OK;
}

extern "C" int wepp_geno_nearest(int device, const wepp_genotypes* g, uint32_t n_a, const uint32_t* keep_bits, uint32_t keep_positions,
                                 int32_t* min_dist, uint32_t* nearest, int32_t* matrix) {
    if (!g || !min_dist || !nearest) return set_error(WEPP_EINVAL, "null argument");
    if (int rc = check_genotypes(g)) return rc;
    if (n_a == 0) return set_error(WEPP_EINVAL, "A is empty: n_a must be at least 1");
    if (n_a >= g->n_items) return set_error(WEPP_EINVAL, "B is empty: n_a = " + std::to_string(n_a) + " of " + std::to_string(g->n_items) + " items");
    const uint32_t n = g->n_items, n_b = n - n_a;
    if (matrix && (u64)n_a * n_b > GENO_MAX_MATRIX_CELLS)
        return set_error(WEPP_ELIMIT, "a matrix of " + std::to_string((u64)n_a * n_b) + " cells exceeds 2^28");
    g_last = GenoTiming{};
    if (int rc = open_device(device)) return rc;
    hipStream_t stream = nullptr;
    wepp_mat::DevBlockCache cache;
    DevPool pool(cache);
    DevEvents<4> ev;
    if (int rc = ev.create()) return rc;

    Columns c;
    HIP_TRY(hipEventRecord(ev[0], stream));
    if (int rc = build_columns(pool, g, 1, nullptr, keep_bits, keep_positions, stream, &c)) return rc;
    HIP_TRY(hipEventRecord(ev[1], stream));
    const u64 bytes = (u64)n * ((c.set_cols[0] + 63) / 64) * 32;
    if (bytes > GENO_PASS_BYTES)
        return set_error(WEPP_ELIMIT, std::to_string(n) + " items of " + std::to_string(c.set_cols[0]) + " columns need " + std::to_string(bytes) +
                                          " bytes of planes, more than a pass holds (" + std::to_string(GENO_PASS_BYTES) + ")");
    PassTables t;
    if (int rc = build_planes(pool, c, g, 0, 1, nullptr, 0, stream, &t)) return rc;
    HIP_TRY(hipEventRecord(ev[2], stream));
    u64* d_best; int32_t* d_matrix = nullptr;
    DEV_GET(pool, d_best, n_a);
    HIP_TRY(hipMemsetAsync(d_best, 0xFF, (size_t)n_a * 8, stream));
    if (matrix) DEV_GET(pool, d_matrix, (size_t)n_a * n_b);
    const uint32_t Ta = (n_a + GENO_TILE - 1) / GENO_TILE, Tb = (n_b + GENO_TILE - 1) / GENO_TILE;
    uint32_t ti = 0, tj = 0;
    auto next = [&](GenoTileJob* j) {
        if (ti >= Ta) return false;
        *j = GenoTileJob{0, ti, tj};
        if (++tj == Tb) { ti++; tj = 0; }
        return true;
    };
    if (int rc = run_tiles(pool, stream, next, [&](const GenoTileJob* d_jobs, uint32_t k) { return launch_geno_tile_nearest(t.dev, d_jobs, k, n_a, d_best, d_matrix, stream); }))
        return rc;
    HIP_TRY(hipEventRecord(ev[3], stream));
    std::vector<u64> best;
    try { best.resize(n_a); } catch (const std::bad_alloc&) { return set_error(WEPP_ENOMEM, "no host memory for the nearest keys"); }
    HIP_TRY(hipMemcpyAsync(best.data(), d_best, (size_t)n_a * 8, hipMemcpyDeviceToHost, stream));
    if (matrix) HIP_TRY(hipMemcpyAsync(matrix, d_matrix, (size_t)n_a * n_b * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (uint32_t a = 0; a < n_a; a++) {
        if (best[a] == ~0ull) return set_error(WEPP_EDEVICE, "no distance was computed for item " + std::to_string(a));
        min_dist[a] = (int32_t)(best[a] >> 32); nearest[a] = (uint32_t)best[a];
    }
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3; i++) HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    g_last.columns_ms = ms[0]; g_last.planes_ms = ms[1]; g_last.pairs_ms = ms[2];
    return WEPP_OK;
}
