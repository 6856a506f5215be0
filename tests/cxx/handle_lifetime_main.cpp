// handle_lifetime_main.cpp -- what a wepp_mat owns goes with it (wepp_amd/csrc/handle.hpp), checked against the
// emulated runtime of tests/cxx/hip_emu, which counts the device blocks, host blocks, streams and events alive and hands
// out streams and events as heap tokens: built with AddressSanitizer, a leak, a second free or a second destroy ends
// the program (tests/test_handle_lifetime.py).
//   (a) a handle deleted straight after construction;
//   (b) a handle that holds everything at least once: uploads, every grow-only buffer (made, regrown, asked for less),
//       every stream and event owner, the clade table, blocks parked in the EPP cache by a DevPool;
//   (c) a handle whose set-up stops at its k-th device allocation, for every k.
#include <cstdio>

#include "../../wepp_amd/csrc/epp_host.hpp"
#include "../../wepp_amd/csrc/handle_setup.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { g_fail++; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static bool nothing_alive() {
    return g_emu_live.dev == 0 && g_emu_live.host == 0 && g_emu_live.streams == 0 && g_emu_live.events == 0 && handles_alive() == 0;
}

// made, regrown (another block, the slack on top), asked for less (nothing moves)
template <typename B>
static void grow_three_times(B& b, bool pinned) {
    long& live = pinned ? g_emu_live.host : g_emu_live.dev;
    const long before = live;
    CHECK(b.reserve(1000, 4, "test") == WEPP_OK);
    CHECK(b.ptr && b.bytes == 1250 && live == before + 1);
    CHECK(b.reserve(5000, 2, "test") == WEPP_OK);
    CHECK(b.ptr && b.bytes == 7500 && live == before + 1);
    memset(b.ptr, 0, b.bytes);
    const void* const p = b.ptr;
    CHECK(b.reserve(100, 4, "test") == WEPP_OK && b.reserve(7500, 4, "test") == WEPP_OK);
    CHECK(b.ptr == p && b.bytes == 7500 && live == before + 1);
}

constexpr size_t kSeedTable = 64;
// device allocations of create_call_resources: d_work, and per lane d_info and the seed table
constexpr long kSetupMallocs = 1 + 2 * wepp_mat::kLanes;

int main() {
    CHECK(nothing_alive());
    // (a)
    {
        wepp_mat* h = new wepp_mat;
        CHECK(handles_alive() == 1);
        delete h;
        CHECK(nothing_alive());
    }
    // (b)
    {
        wepp_mat* h = new wepp_mat;
        CHECK(upload(h, std::vector<uint32_t>{0, 1, 2}, &h->dev.node_woff) == WEPP_OK);
        CHECK(upload(h, std::vector<uint32_t>(), &h->dev.words) == WEPP_OK);          // (an empty array is a block too)
        CHECK(upload(h, std::vector<uint32_t>(1000, 7u), &h->dev.parent_dfs) == WEPP_OK);
        uint8_t* raw = nullptr;
        CHECK(dev_alloc(h, 100, &raw) == WEPP_OK && raw);
        CHECK(g_emu_live.dev == 4 && h->stats.device_bytes == 16 + 16 + 4000 + 100);   // (a block has 16 bytes at least)
        CHECK(create_call_resources(h, kSeedTable) == WEPP_OK);
        CHECK(g_emu_live.dev == 4 + kSetupMallocs && g_emu_live.host == wepp_mat::kLanes);
        CHECK(g_emu_live.streams == wepp_mat::kLanes * MAX_STREAMS);
        CHECK(g_emu_live.events == wepp_mat::kLanes * (MAX_STREAMS + 3) + 2 * wepp_mat::kRing);
        CHECK(create_pipeline(h) == WEPP_OK);
        CHECK(create_pipeline(h) == WEPP_OK);                                          // (the second call finds everything made)
        CHECK(g_emu_live.streams == wepp_mat::kLanes * (MAX_STREAMS + 3));
        CHECK(g_emu_live.events == wepp_mat::kLanes * (MAX_STREAMS + 3) + 2 * wepp_mat::kRing + 6 * wepp_mat::kPipeMax);
        CHECK(h->lane[1].side[MAX_STREAMS - 1] && h->lane[1].join_ev[MAX_STREAMS - 1] && (hipEvent_t)h->lane[1].info_ev && h->pipe_out[4 * wepp_mat::kPipeMax - 1]);
        grow_three_times(h->io_in, false);
        grow_three_times(h->io_out, false);
        grow_three_times(h->pin, true);
        grow_three_times(h->pin_out, true);
        grow_three_times(h->d_plan_of, false);
        grow_three_times(h->d_wsid_of, false);
        for (PlaceLane& L : h->lane) {
            grow_three_times(L.ws, false);
            grow_three_times(L.part, false);
        }
        CHECK(hipMalloc((void**)&h->clade_tab.ptr, 256) == hipSuccess && hipMalloc((void**)&h->nbr_dfs_end.ptr, 256) == hipSuccess);
        long parked = 0;
        {
            DevPool pool(h->epp_cache);
            uint32_t* a = nullptr;
            uint8_t* b = nullptr;
            CHECK(pool.get(&a, 100) == hipSuccess && pool.get(&b, 5000) == hipSuccess && a && b);
            parked = 2;
        }
        CHECK(h->epp_cache.blocks.size() == (size_t)parked);
        {
            DevPool pool(h->epp_cache);                                                // (takes the block of the first call back out)
            uint32_t* a = nullptr;
            const long dev = g_emu_live.dev;
            CHECK(pool.get(&a, 100) == hipSuccess && g_emu_live.dev == dev && h->epp_cache.blocks.size() == 1);
        }
        CHECK(h->epp_cache.blocks.size() == 2);
        CHECK(g_emu_live.dev == 4 + kSetupMallocs + 4 + 2 * wepp_mat::kLanes + 2 + parked && g_emu_live.host == wepp_mat::kLanes + 2);
        CHECK(handles_alive() == 1);
        delete h;
        CHECK(nothing_alive());
    }
    // (c)
    for (long k = 0; k <= kSetupMallocs; k++) {
        wepp_mat* h = new wepp_mat;
        g_emu_malloc_budget = k;
        const int rc = create_call_resources(h, kSeedTable);
        g_emu_malloc_budget = -1;
        CHECK(k == kSetupMallocs ? rc == WEPP_OK : rc != WEPP_OK);
        CHECK(g_emu_live.dev == k);
        // (stopped at the second lane's counters, the first lane's streams and events exist and the ring does not)
        if (k == 2) CHECK(g_emu_live.streams == MAX_STREAMS && g_emu_live.events == MAX_STREAMS + 3 && g_emu_live.host == 1);
        delete h;
        CHECK(nothing_alive());
    }
    if (g_fail) return 1;
    printf("ok handle lifetime: empty, full and %ld interrupted set-ups leave nothing alive\n", kSetupMallocs + 1);
    return 0;
}
