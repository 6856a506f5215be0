// The host side of a Fitch-Sankoff plan (wepp_amd/csrc/fitch_plan.hpp) and the two ways device tables are made
// (handle.hpp: DevMem::alloc, upload_whole), built against the emulated runtime of tests/cxx/hip_emu, plain and under
// AddressSanitizer + UBSan, by tests/test_fitch_plan_host.py.  Prints "ok <checks>", or the failed check and exit status 1.
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../wepp_amd/csrc/fitch_plan.hpp"
#include "../../wepp_amd/csrc/handle.hpp"

namespace {
int g_checks = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
typedef std::vector<uint32_t> V;

int owners() {
    const uint32_t a[5] = {1, 2, 3, 4, 5}, b[3] = {7, 8, 9};
    DevMem<uint32_t> d;
    const long live = g_emu_live.dev;
    g_emu_malloc_budget = 0;
    CHECK(upload_whole(d, a, 5, "a") == WEPP_ENOMEM && !d.ptr && g_emu_live.dev == live);
    CHECK(d.alloc(5, "a") == WEPP_ENOMEM && !d.ptr && g_emu_live.dev == live && strstr(wepp_last_error(), "hipMalloc a: "));
    g_emu_malloc_budget = -1;
    CHECK(upload_whole(d, a, 5, "a") == WEPP_OK && d.ptr && g_emu_live.dev == live + 1 && !memcmp(d.ptr, a, sizeof a));
    CHECK(upload_whole(d, b, 3, "b") == WEPP_OK && g_emu_live.dev == live + 1 && !memcmp(d.ptr, b, sizeof b));
    g_emu_malloc_budget = 0;           // a publish that fails leaves the table that is there
    CHECK(upload_whole(d, a, 5, "a") == WEPP_ENOMEM && g_emu_live.dev == live + 1 && !memcmp(d.ptr, b, sizeof b));
    g_emu_malloc_budget = -1;
    // alloc(0): the old block goes, 16 bytes come (under ASan a shorter block ends before the last word of its guard)
    CHECK(d.alloc(0, "none") == WEPP_OK && d.ptr && g_emu_live.dev == live + 1);
    for (uint32_t i = 0; i < 4; i++) d.ptr[i] = i;
    for (uint32_t i = 4; i < 4 + EMU_GUARD_BYTES / 4; i++) CHECK(d.ptr[i] == EMU_FILL);
    d.reset();
    CHECK(!d.ptr && g_emu_live.dev == live);
    return 0;
}

int forms() {
    for (int m = 0; m < 16; m++) {
        const bool tree = m & 1, scores = m & 2, dfs = m & 4, empty = m & 8;
        bool sets_ok = tree;               // the run's own sequence of decisions, restated
        if (scores) sets_ok = false;
        if (empty) sets_ok = false;
        bool levels = sets_ok;
        if (dfs) levels = false;
        FitchForm f{};
        CHECK(fitch_choose_form(tree, scores, dfs, empty, 3, &f) == WEPP_OK && f.levels == levels && f.sets_ok == sets_ok);
        CHECK(fitch_choose_form(tree, scores, dfs, empty, FITCH_MAX_DEPTH, &f) == WEPP_OK);
        CHECK(fitch_choose_form(tree, scores, dfs, empty, FITCH_MAX_DEPTH + 1, &f) == (levels ? WEPP_OK : WEPP_ELIMIT));
    }
    CHECK(FITCH_MAX_DEPTH == 140 && strstr(wepp_last_error(), "tree depth 141 exceeds the LDS stack (140)"));
    return 0;
}

// a tree by its parent array, nodes numbered in pre-order
int tables(const V& parent) {
    const uint32_t N = (uint32_t)parent.size();
    V depth(N, 0), bfs2dfs(N), dfs2bfs(N);
    for (uint32_t d = 1; d < N; d++) depth[d] = depth[parent[d]] + 1;
    const uint32_t max_depth = *std::max_element(depth.begin(), depth.end());
    std::iota(bfs2dfs.begin(), bfs2dfs.end(), 0u);
    std::stable_sort(bfs2dfs.begin(), bfs2dfs.end(), [&](uint32_t a, uint32_t b) { return depth[a] < depth[b]; });
    for (uint32_t b = 0; b < N; b++) dfs2bfs[bfs2dfs[b]] = b;
    auto ancestor = [&](uint32_t x, uint32_t k) { while (depth[x] > k) x = parent[x]; return x; };
    for (long hook : {-1L, 0L, 1L, 2L, 3L, 5L, (long)N, (long)N + 7, 0xFFFFFFFFL}) {
        const FitchChunks t = fitch_build_chunks(N, hook, max_depth, parent.data(), depth.data());
        const uint32_t C = hook < 0 ? 1 : (uint32_t)std::max(1L, std::min(hook, (long)N));
        CHECK(t.C == C && t.D == max_depth + 1 && t.start.size() == C + 1 && t.depth.size() == C + 1 && t.min.size() == C && t.open.size() == (size_t)(C + 1) * t.D);
        for (uint32_t c = 0; c <= C; c++) {
            CHECK(t.start[c] == (uint64_t)N * c / C);
            const uint32_t x = c < C ? t.start[c] : N - 1;
            if (c == C && N == 1) { CHECK(t.depth[c] == 1 && t.open[(size_t)c * t.D] == 0); continue; }
            CHECK(t.depth[c] == depth[x]);
            for (uint32_t k = 0; k < depth[x]; k++) CHECK(t.open[(size_t)c * t.D + k] == ancestor(x, k));
        }
        for (uint32_t c = 0; c < C; c++) CHECK(t.min[c] == *std::min_element(depth.begin() + t.start[c], depth.begin() + t.start[c + 1]));
    }
    const FitchLevelTables l = fitch_build_levels(N, parent.data(), depth.data(), dfs2bfs.data());
    V cuts;
    for (uint32_t b = 0; b < N; b++)
        if (b == 0 || depth[bfs2dfs[b]] != depth[bfs2dfs[b - 1]]) cuts.push_back(b);
    cuts.push_back(N);
    CHECK(l.level_off == cuts && l.level_off.size() == (size_t)max_depth + 2 && l.coff.size() == (size_t)N + 1 && l.par.size() == N);
    for (uint32_t i = 0; i < N; i++) {
        CHECK(l.coff[i] <= l.coff[i + 1] && l.coff[i + 1] <= N);
        for (uint32_t b = 1; b < N; b++) CHECK((l.par[b] == i) == (l.coff[i] <= b && b < l.coff[i + 1]));
    }
    for (uint32_t b = 1; b < N; b++) CHECK(l.par[b] == dfs2bfs[parent[bfs2dfs[b]]]);
    return 0;
}

int shapes() {
    const size_t ample = (size_t)1 << 40;
    FitchShape s = fitch_run_shape(1000, 700, true, 0, 0, 0, 0, -1);
    CHECK(s.rows_per_batch == 256 && s.nbatches == 3 && s.part_bytes == 0 && s.group == 1 && s.tables_need == 256000);
    s = fitch_run_shape(1000, 700, true, 0, 0, ample, 0, -1);
    CHECK(s.group == 3 && s.tables_need == 768000);
    CHECK(fitch_run_shape(1000, 700, true, 0, 0, ample, 0, 2).group == 2 && fitch_run_shape(1000, 700, true, 0, 0, ample, 0, 0).group == 1);
    CHECK(fitch_run_shape(1000, 700, true, 0, 0, ample, 0, 9).group == 3);        // the hook can only lower the group
    // stack forms: 64 rows a batch; per batch 4096 * 64 + 2 * 10240 = 282624 bytes, 4 batches of 200 rows
    s = fitch_run_shape(4096, 200, false, 2, 5, 1200000, 0, -1);
    CHECK(s.rows_per_batch == 64 && s.nbatches == 4 && s.part_bytes == 10240 && s.group == 2 && s.tables_need == 2 * 262144);
    CHECK(fitch_run_shape(4096, 200, false, 2, 5, 1000000, 0, -1).group == 1);
    CHECK(fitch_run_shape(4096, 200, false, 2, 5, 1000000, 200000, -1).group == 2);
    CHECK(fitch_run_shape(4096, 200, false, 2, 5, 2 * 282624 * 4, 0, -1).group == 4 && fitch_run_shape(4096, 200, false, 2, 5, 2 * 282624 * 4 - 2, 0, -1).group == 3);
    return 0;
}
}  // namespace

int main() {
    if (owners() || forms() || shapes()) return 1;
    for (const V& parent : {V{0}, V{0, 0, 1, 2}, V{0, 0, 0, 0, 0}, V{0, 0, 1, 1, 3, 0, 5, 5, 5, 8, 0, 10}})
        if (tables(parent)) return 1;
    if (g_emu_live.dev != 0) { printf("%ld device blocks left\n", g_emu_live.dev); return 1; }
    printf("ok %d\n", g_checks);
    return 0;
}
