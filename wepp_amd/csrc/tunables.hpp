// tunables.hpp -- every environment knob of the placement path, read ONCE when a handle is created (wepp_mat::tun)
// or once per flatten (FlattenOptions), clamped to what the kernels take.  None of them changes a result: they are
// A/B aids, profiling aids and test hooks (DESIGN.md "Diagnostic switches").  The hot call path reads struct fields,
// never the environment.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "device_mat.hpp"
#include "flatten_options.hpp"

namespace wepp {


struct PlaceTunables {
    // walks
    bool walk = true;                    // WEPP_WALK=0: every read is placed by sweeps
    uint32_t walk_eager_nodes = WALK_EAGER_MAX_NODES;   // WEPP_WALK_EAGER_NODES
    uint32_t walk_max_events = WALK_MAX_EVENTS;         // WEPP_WALK_MAX_EVENTS: events from which a walk is cut into jobs
    bool ww_fixed = false;               // WEPP_WW_BLOCK_MAX_SMALL / _BIG given: reads per routing block listed for k_walk_wave (default: all or none, by the previous call's counts)
    uint32_t ww_block_max_small = 0xFFFFFFFFu, ww_block_max_big = 0xFFFFFFFFu;
    // launch structure of a call (capi.cpp: place_device)
    bool step_unfused = false;           // WEPP_STEP_UNFUSED=1: plain walks, k_walk_wave and the 8-entry job class as three blind launches behind k_route instead of k_step (the form before it; results identical)
    bool step_groups = true;             // WEPP_STEP_GROUPS=0: the plain walkers of k_step lane = read (walk_body) instead of by lane groups (place_dev.hpp: group_read; results identical)
    bool scatter_blind = false;          // WEPP_SCATTER_BLIND=1: k_scatter launched blind behind the counters' copy in every call, whether or not a launch reads its lists (the form before the lists became lazy; results identical)
    bool info_copy = false;              // WEPP_INFO_COPY=1: the routing counters reach the host by a copy on the plan stream and an event in every call, instead of k_step's report (the form before the report, and the one every call without k_step keeps; results identical)
    bool stamp_records = false;          // WEPP_STAMP_RECORDS=1: the two time stamps of a call as event records of their own, instead of stop events of k_route's and k_step's launches (the form before; results and the span's meaning identical)
    // seeds: whole-genome samples
    bool seed = true;                   // WEPP_SEED=0: whole-genome samples take the tile sweeps
    bool seed_heavy = true;              // WEPP_SEED_HEAVY=0: no second pass (a sample's workgroup evaluates every chunk it must itself)
    uint32_t seed_min_hard = SEED_MIN_HARD;          // WEPP_SEED_MIN_HARD
    uint32_t seed_min_nodes = SEED_MIN_STREAM_NODES; // WEPP_SEED_MIN_NODES
    // host pipeline of wepp_place_batch
    uint32_t pipe_sub_batches = 0;       // WEPP_PIPE_SUBBATCHES
    uint32_t pipe_min_chunks = 4;        // WEPP_PIPE_MIN_CHUNKS: copy chunks of a host-buffer batch (rounded up to a multiple of its sub-batches)
    uint32_t host_threads = 0;           // WEPP_HOST_THREADS (0: cores this process may use / handles alive)
    // diagnostics
    bool debug_plans = false, debug_timing = false, walk_debug = false;

    static PlaceTunables from_env() {
        PlaceTunables t;
        t.walk = env::flag("WEPP_WALK", true);
        t.walk_eager_nodes = (uint32_t)env::u64("WEPP_WALK_EAGER_NODES", WALK_EAGER_MAX_NODES, 0, 0xFFFFFFFFu);
        t.walk_max_events = (uint32_t)env::u64("WEPP_WALK_MAX_EVENTS", WALK_MAX_EVENTS, 0, 0xFFFFu);
        t.ww_fixed = env::is_set("WEPP_WW_BLOCK_MAX_SMALL") || env::is_set("WEPP_WW_BLOCK_MAX_BIG");
        t.ww_block_max_small = (uint32_t)env::u64("WEPP_WW_BLOCK_MAX_SMALL", 0xFFFFFFFFu, 0, 0xFFFFFFFFu);
        t.ww_block_max_big = (uint32_t)env::u64("WEPP_WW_BLOCK_MAX_BIG", 0xFFFFFFFFu, 0, 0xFFFFFFFFu);
        t.step_unfused = env::is_set("WEPP_STEP_UNFUSED") && env::flag("WEPP_STEP_UNFUSED", false);
        t.step_groups = env::flag("WEPP_STEP_GROUPS", true);
        t.scatter_blind = env::is_set("WEPP_SCATTER_BLIND") && env::flag("WEPP_SCATTER_BLIND", false);
        t.info_copy = env::is_set("WEPP_INFO_COPY") && env::flag("WEPP_INFO_COPY", false);
        t.stamp_records = env::is_set("WEPP_STAMP_RECORDS") && env::flag("WEPP_STAMP_RECORDS", false);
        t.seed = env::flag("WEPP_SEED", true);
        t.seed_heavy = env::flag("WEPP_SEED_HEAVY", true);
        t.seed_min_hard = (uint32_t)env::u64("WEPP_SEED_MIN_HARD", SEED_MIN_HARD, 0, 0xFFFFu);
        t.seed_min_nodes = (uint32_t)env::u64("WEPP_SEED_MIN_NODES", SEED_MIN_STREAM_NODES, 0, 0xFFFFFFFFu);
        t.pipe_sub_batches = (uint32_t)env::u64("WEPP_PIPE_SUBBATCHES", 0, 1, 8);
        t.pipe_min_chunks = (uint32_t)env::u64("WEPP_PIPE_MIN_CHUNKS", 4, 1, 64);
        t.host_threads = (uint32_t)env::u64("WEPP_HOST_THREADS", 0, 1, 256);
        t.debug_plans = env::is_set("WEPP_DEBUG_PLANS");
        t.debug_timing = env::is_set("WEPP_DEBUG_TIMING");
        t.walk_debug = env::is_set("WEPP_WALK_DEBUG");
        return t;
    }
};

}  // namespace wepp
