// The launch planner of a placement call (wepp_amd/csrc/launch_plan.hpp) on a planning problem read from standard input,
// built against the emulated runtime of tests/cxx/hip_emu (the planner makes no HIP call; device_mat.hpp names HIP's
// types).  A program of its own, built plain and under AddressSanitizer + UBSan by tests/test_sweep_cases.py.
//
// Input, whitespace-separated unsigned numbers:
//   T walking fuse_windows
//   bm_words max_pos n_streams seed_chunks wc_windows
//   n_streams x (NB ncp cp_stride bytes)
//   n_wstreams, then n_wstreams x (NB ncp cp_stride bytes)
//   n, then n x (plan id, count, maxk)
// Output: the `[plan]` line of every tile plan, as place_device prints it under WEPP_DEBUG_PLANS, and a `[launch]` line
// with the partition and the totals; or, when the planner refuses, "error <code>: <message>" and exit status 3.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../wepp_amd/csrc/launch_plan.hpp"

using namespace wepp;

namespace {
bool rd(unsigned long long& v) { return scanf("%llu", &v) == 1; }
bool rd32(uint32_t& v) { unsigned long long x; if (!rd(x) || x > 0xFFFFFFFFull) return false; v = (uint32_t)x; return true; }
bool rd_geoms(std::vector<DevStream>& g, std::vector<uint64_t>& bytes) {
    bytes.resize(g.size());
    for (size_t i = 0; i < g.size(); i++) {
        unsigned long long b;
        g[i] = DevStream{};
        if (!rd32(g[i].NB) || !rd32(g[i].ncp) || !rd32(g[i].cp_stride) || !rd(b)) return false;
        bytes[i] = b;
    }
    return true;
}
void list(const char* what, const uint32_t* idx, uint32_t n) {
    printf(" %s=", what);
    for (uint32_t i = 0; i < n; i++) printf("%s%u", i ? "," : "", idx[i]);
}
}  // namespace

int main() {
    DevMAT m{};
    uint32_t T, walking, fuse, n_ws, n;
    if (!rd32(T) || !rd32(walking) || !rd32(fuse)) return 2;
    if (!rd32(m.bm_words) || !rd32(m.max_pos) || !rd32(m.n_streams) || !rd32(m.seed_chunks) || !rd32(m.wc_windows)) return 2;
    if (m.n_streams < 1 || m.n_streams > MAX_STREAMS) return 2;
    std::vector<DevStream> streams(m.n_streams);
    std::vector<uint64_t> sbytes, wbytes;
    if (!rd_geoms(streams, sbytes) || !rd32(n_ws) || n_ws > MAX_WINDOWS) return 2;
    std::vector<DevStream> wstreams(n_ws);
    if (!rd_geoms(wstreams, wbytes) || !rd32(n)) return 2;
    std::vector<uint32_t> info(TI_WORDS, 0u);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t id, count, maxk;
        if (!rd32(id) || !rd32(count) || !rd32(maxk) || id >= MAX_PLANS) return 2;
        info[TI_COUNT + id] = count;
        info[TI_MAXK + id] = maxk;
    }
    // (TI_OFF as k_scatter and place_device form it: the exclusive prefix sum of the counts)
    uint32_t off = 0;
    for (uint32_t t = 0; t < MAX_PLANS; t++) { info[TI_OFF + t] = off; off += info[TI_COUNT + t]; }
    info[TI_OFF + MAX_PLANS] = off;
    std::vector<LaunchPlan> lp(1);
    const int rc = plan_launches(info.data(), T, walking != 0, fuse != 0, m, streams.data(), sbytes.data(), wstreams.data(), wbytes.data(), n_ws, lp[0]);
    if (rc != WEPP_OK) {
        printf("error %d: %s\n", rc, wepp_last_error());
        return 3;
    }
    const LaunchPlan& p = lp[0];
    for (uint32_t i = 0; i < p.np; i++) print_plan_line(stdout, p.plans[i]);
    // the rest of the plan in one line: the partition (indices of the `[plan]` lines above, in launch order) and the totals
    printf("[launch]");
    list("plain", p.order, p.n_plain);
    list("windows", p.wins, p.n_wins);
    list("others", p.others, p.n_other);
    printf(" arena=%u@%zu seeds=%u part_total=%zu walk_reads=%llu passes=%llu bytes=%llu\n", p.arena_n, p.arena_part, p.seed_n, p.part_total,
           (unsigned long long)p.walk_reads, (unsigned long long)p.passes, (unsigned long long)p.bytes);
    return 0;
}
