// handle.hpp -- the object behind wepp_mat_t and the small helpers the C-ABI translation units (capi.cpp,
// place_batch.cpp and the *_capi.cpp of the entry points) share.  It compiles against the emulated runtime of tests/cxx/hip_emu too:
// tests/epp_emu.py runs the entry points' own host code on a handle made there.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/wepp_place.h"
#include "device_mat.hpp"
#include "errors.hpp"
#include "flatmat.hpp"
#include "host_pool.hpp"
#include "tunables.hpp"

using namespace wepp;

namespace wepp {

inline int hip_fail(hipError_t e, const char* what) {
    return set_error(WEPP_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                      \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_fail(_e, #expr);  \
    } while (0)

// a call that returns a WEPP_* code: anything but WEPP_OK is the caller's return value too
#define WEPP_TRY(expr)                     \
    do {                                   \
        const int _rc = (expr);            \
        if (_rc != WEPP_OK) return _rc;    \
    } while (0)

// ---- owners of HIP resources: each frees what it holds when it goes; none can be copied.  A handle's members are
// destroyed behind the body of ~wepp_mat(), which has selected the handle's device. ----
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

// one block of device memory, or (pinned) of host memory from hipHostMalloc: filled in by whoever allocates it
template <typename T = void> struct DevMem : NoCopy {
    T* ptr = nullptr;
    bool pinned = false;
    explicit DevMem(bool pinned_host = false) : pinned(pinned_host) {}
    ~DevMem() { reset(); }
    void reset() {
        if (ptr) (void)(pinned ? hipHostFree(ptr) : hipFree(ptr));
        ptr = nullptr;
    }
    operator T*() const { return ptr; }
    // gives back what it holds and takes `bytes` bytes, at least 16 / `count` elements (bytes for T = void)
    int alloc_bytes(size_t bytes, const char* what) {
        reset();
        bytes = std::max<size_t>(bytes, 16);
        const hipError_t e = pinned ? hipHostMalloc((void**)&ptr, bytes) : hipMalloc((void**)&ptr, bytes);
        if (e == hipSuccess) return WEPP_OK;
        ptr = nullptr;
        return set_error(WEPP_ENOMEM, std::string(pinned ? "hipHostMalloc " : "hipMalloc ") + what + ": " + hipGetErrorString(e));
    }
    int alloc(size_t count, const char* what) { return alloc_bytes(count * sizeof(std::conditional_t<std::is_void_v<T>, char, T>), what); }
};

// A table an owner keeps between calls is made whole or not at all: filled in a block of its own and swapped in, the
// block it replaces freed behind the swap.  On any failure `dst` is as it was: an owner is null or holds a table
// that was written completely.
template <typename T>
inline int upload_whole(DevMem<T>& dst, const T* src, size_t count, const char* what) {
    DevMem<T> fresh(dst.pinned);
    WEPP_TRY(fresh.alloc(count, what));
    const hipError_t e = count ? hipMemcpy(fresh, src, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) return set_error(WEPP_EDEVICE, std::string("upload of ") + what + ": " + hipGetErrorString(e));
    std::swap(dst.ptr, fresh.ptr);
    return WEPP_OK;
}

// A grow-only buffer of a handle, in device or in pinned host memory: kept while it holds `need` bytes; else freed --
// behind a device-wide synchronisation: work in flight may still use it, hipFree waits for the device anyway, and a
// buffer regrows only while its handle warms up -- and allocated again with need / slack bytes to spare.
template <typename T = void> struct GrowBuf : DevMem<T> {
    size_t bytes = 0;
    using DevMem<T>::DevMem;
    int reserve(size_t need, size_t slack, const char* what) {
        if (need <= bytes) return WEPP_OK;
        if (this->ptr) HIP_TRY(hipDeviceSynchronize());
        bytes = 0;
        const size_t want = need + need / slack;
        WEPP_TRY(this->alloc_bytes(want, what));
        bytes = want;
        return WEPP_OK;
    }
};

// device blocks that live as long as the handle (upload() below adds to them)
struct DevAllocs : NoCopy {
    std::vector<void*> blocks;
    ~DevAllocs() { for (void* p : blocks) (void)hipFree(p); }
    void push_back(void* p) { blocks.push_back(p); }
    auto begin() const { return blocks.begin(); }
    auto end() const { return blocks.end(); }
};

// N events / N streams; create() makes the ones not made yet, the destructor destroys those that were made
template <int N> struct DevEvents : NoCopy {
    hipEvent_t ev[N] = {};
    int n = 0;                         // created so far
    ~DevEvents() { while (n > 0) (void)hipEventDestroy(ev[--n]); }
    int create(unsigned flags = 0) {       // (0: hipEventDefault, what hipEventCreate makes)
        for (; n < N; n++) { hipEvent_t& x = ev[n]; HIP_TRY(hipEventCreateWithFlags(&x, flags)); }
        return WEPP_OK;
    }
    hipEvent_t operator[](size_t i) const { return ev[i]; }
    template <int M = N, typename = std::enable_if_t<M == 1>> operator hipEvent_t() const { return ev[0]; }   // (a single event stands for itself)
};
// (create() is handed the runtime's two stream calls -- handle_setup.hpp: hipStreamCreateWithFlags, hipStreamDestroy --
// so that this header asks for no stream call itself: the entry points that only borrow a handle, and the emulated
// runtime they are tested against, need none)
template <int N> struct DevStreams : NoCopy {
    hipStream_t st[N] = {};
    int n = 0;
    hipError_t (*destroy)(hipStream_t) = nullptr;
    ~DevStreams() { while (n > 0) (void)destroy(st[--n]); }
    int create(hipError_t (*make)(hipStream_t*, unsigned), hipError_t (*unmake)(hipStream_t), unsigned flags) {
        destroy = unmake;
        for (; n < N; n++) { hipStream_t& x = st[n]; HIP_TRY(make(&x, flags)); }
        return WEPP_OK;
    }
    hipStream_t operator[](size_t i) const { return st[i]; }
};

// handles alive in this process: a handle's host workers are its share of the cores the process may use.  Counted by a
// member, so that wepp_mat keeps its implicit constructor (`new wepp_mat()` zeroes the object, padding included).
inline std::atomic<uint32_t> g_handles_alive{0};
inline uint32_t handles_alive() { return g_handles_alive.load(std::memory_order_relaxed); }
struct HandleCount : NoCopy {
    HandleCount() { g_handles_alive.fetch_add(1, std::memory_order_relaxed); }
    ~HandleCount() { g_handles_alive.fetch_sub(1, std::memory_order_relaxed); }
};

}  // namespace wepp

// a device block of the handle's cache: its size and the most bytes a call ever asked of it (the rest is rounding).
// `asked` is not used by the product: the emulation's guard check (tests/cxx/epp_emu.cpp) looks for stores past it.
struct DevBlock { void* ptr; size_t bytes, asked; };

// What ONE placement call in flight needs of its own: two device blocks, routing counters, the side streams its launch
// chains run on.  A handle has two: the sub-batches of wepp_place_batch alternate between them, so that the routing
// of sub-batch k+1 (kernels, a device-to-host copy, the host's poll) overlaps the walks of sub-batch k, each lane's
// work ordered on the lane's own compute stream.  wepp_place_batch_device uses lane 0.
struct PlaceLane {
    // Two grow-only blocks, sized at the two moments a call knows the sizes (capi.cpp: carve_workspace, reserve_partials).
    // ws: the regions sized by the number of reads alone -- read list, root scores, routing arrays, walk lists, blind job
    // tables, sort keys and scratch.  Grown before k_route, which writes into it: it does not move during a call.
    GrowBuf<> ws;
    // part: what is sized from the routing counters -- 12 bytes per (chunk, read) of every sweep plan and, behind them,
    // the job tables and partials of the chunked walks the host plans itself.  Grown behind the planner (capi.cpp: reserve_partials), before
    // anything of the call has touched it.
    GrowBuf<> part;
    DevMem<uint32_t> d_info;          // two sets of tier_info (TI_WORDS each, used alternately: k_route clears the other one) followed by blk_counts
    uint32_t info_idx = 0;            // the set the next call uses (zero: cleared at creation or by the previous call's k_route)
    // the host's copy of tier_info AND the report block of k_step (info_wait.hpp: info_block_words): coherent, mapped
    // host memory -- TI_WORDS counters and, on a cache line of its own, the sequence word of the call that wrote them.
    // A call without a report fills the counters by a copy on the plan stream and leaves the sequence word alone.
    DevMem<uint32_t> h_info{true};
    uint32_t* d_report = nullptr;     // the same block as the device addresses it (not a block of its own: nothing to free)
    uint32_t info_seq = 0;            // sequence number of the lane's last call that asked for a report (never 0 once one has)
    // the launch chains of a call are independent: they run concurrently on side streams
    DevStreams<MAX_STREAMS> side;
    DevEvents<1> fork_ev;
    DevEvents<MAX_STREAMS> join_ev;
    DevEvents<1> route_ev;            // behind k_route: the plain walks start from here on their side stream, before the host has the counters
    DevEvents<1> info_ev;             // behind the copy of tier_info to h_info: the host polls it, whatever is queued behind the copy
    // k_seed's table of samples handed to its second pass (seed_kernels.hip), zero between calls.  One per lane: a
    // record names a read of ITS sub-batch, and the finalize kernel writes into its lane's result arrays and clears the
    // count -- the seed chains of two lanes may run at the same time.
    DevMem<> d_seed_heavy;
};

// Which of a lane's side streams (and join events, same index) a launch chain of place_device runs on (capi.cpp: the
// stages route_and_launch_blind, launch_late_classes and the launch_* chains behind the planner).  The values are
// the ones every measurement was taken with and must not change.  The plans launched on their own (dense, out-of-LDS,
// window plans beyond MAX_WINDOWS) take side[k % OTHER_SIDE_STREAMS] in turn, so some streams serve twice: stream 10 is
// the 16-entry plain walk class AND the fused window plans, stream 9 is the plan stream AND the tenth such plan (11 and
// 12, seeds and arena, the twelfth and thirteenth).  Chains that share a stream run one behind the other, no more.
constexpr uint32_t SIDE_WAVE = MAX_STREAMS - 1;        // k_walk_wave of WEPP_STEP_UNFUSED=1 (route_and_launch_blind)
constexpr uint32_t SIDE_JOBS8 = MAX_STREAMS - 2;       // the 8-entry job class, blind or planned
constexpr uint32_t SIDE_JOBS16 = MAX_STREAMS - 3;      // the 16-entry job class
constexpr uint32_t SIDE_WALK16 = MAX_STREAMS - 6;      // the plain walks of 9 - 16 entries
constexpr uint32_t SIDE_PLAN = MAX_STREAMS - 7;        // everything the host sizes: the counters' copy, k_scatter, the fused sweeps
constexpr uint32_t OTHER_SIDE_STREAMS = MAX_STREAMS - 3;   // streams 0 .. 12: the plans launched on their own; the three behind them belong to the walks
constexpr uint32_t SIDE_ARENA = OTHER_SIDE_STREAMS - 1;    // window-crown sweeps (k_sweep_arena)
constexpr uint32_t SIDE_SEED = OTHER_SIDE_STREAMS - 2;     // whole-genome samples (k_seed)
constexpr uint32_t SIDE_WINDOWS = OTHER_SIDE_STREAMS - 3;  // the fused window plans (k_sweep_windows)
static_assert(SIDE_WALK16 == 10 && SIDE_WINDOWS == 10 && SIDE_PLAN == 9 && SIDE_SEED == 11 && SIDE_ARENA == 12, "the side streams keep their numbers");

struct wepp_mat : NoCopy {
    // the members below free what they hold behind this body, on the handle's device
    ~wepp_mat() { (void)hipSetDevice(device); }
    HandleCount alive;
    static constexpr uint32_t kLanes = 2;
    int device = 0;
    DevMAT dev{};
    std::vector<DevStream> streams;
    std::vector<DevWalk> walks;       // position index + range-query structures of every stream (k_walk)
    uint64_t wc_nodes = 0;            // nodes of all window crowns (the arena of slot WC_SLOT)
    uint32_t wc_count = 0;            // window crowns built
    PlaceTunables tun;                // the environment's knobs, read once when the handle was created (tunables.hpp)
    int use_walk = 1;                 // reads with few entries walk their own events (WEPP_WALK=0: sweeps only)
    int use_seeds = 1;                // whole-genome samples go by chunk signatures (WEPP_SEED=0: tile sweeps)
    std::atomic<uint32_t> job_events[2] = {{WALK_JOB_EVENTS}, {WALK_JOB_EVENTS}};   // events per job of the chunked classes in the next call (a hint: the two launch threads of a pipelined call read and write it freely)
    int walk_ok = 1;                  // 0: a stream is too large for the walk's packed interval stack (sweeps only)
    DevMem<unsigned long long> d_work;      // [WALK_COUNTERS] loop iterations of the walks, [WALK_COUNTERS] bytes the walks / seeds asked memory for,
                                            // [D_WORK_EXTRA] seeded samples, chunks they evaluated, chunks in all, most per sample, histogram -- since the last timing reset
    static constexpr uint32_t D_WORK_EXTRA = 16;
    static constexpr size_t D_WORK_BYTES = (2 * WALK_COUNTERS + D_WORK_EXTRA) * sizeof(unsigned long long);
    std::vector<uint64_t> stream_bytes;
    std::vector<DevStream> wstreams;  // window streams (PLAN_WIN)
    const DevStream* d_wstreams = nullptr;  // ... and the same records on the device (k_sweep_windows names a stream by its index)
    std::vector<uint64_t> wstream_bytes;
    wepp_mat_stats stats{};
    std::vector<uint32_t> bfs2id;
    std::vector<uint32_t> dfs2id;     // caller id of the node with pre-order (arena) index k
    // EPP event stream (flatmat.hpp), resident next to the sweep streams
    const uint32_t* epp_word = nullptr;
    const uint32_t* epp_node = nullptr;
    uint64_t epp_events = 0;
    // device buffers of wepp_epp_map kept between calls (gigabytes at 16 M nodes: a hipMalloc of that size costs
    // tens of milliseconds); a call takes the blocks that fit and hands everything back when it returns.  Freed
    // with the handle (~wepp_mat() has selected the device by then).
    struct DevBlockCache : NoCopy {
        std::vector<DevBlock> blocks;
        ~DevBlockCache() { for (auto& b : blocks) (void)hipFree(b.ptr); }
    } epp_cache;
    // wepp_epp_neighbors (neighbors_capi.cpp): one past the last pre-order index of every subtree, derived from
    // parent_dfs and uploaded by the first call; columns per pass forced by WEPP_NBR_PASS_COLS
    // (-1: not read yet, 0: sized by the memory budget)
    DevMem<uint32_t> nbr_dfs_end;
    int nbr_pass_cols = -1;
    // wepp_mat_set_clades (clades_capi.cpp): [columns][2][N] nearest annotated ancestor of every DFS node, excluding /
    // including the node; replaced by every call, freed with the handle (in `allocs` it would pile up)
    uint32_t clade_columns = 0;
    DevMem<uint32_t> clade_tab;
    std::vector<uint32_t> epp_pending;   // EPP lists of the last wepp_epp_map that did not fit the caller's buffer (wepp_epp_fetch_lists)
    DevAllocs allocs;                 // the tree's arrays and whatever else upload() / dev_alloc() made
    uint32_t tile_reads = 64;
    int use_crowns = 1;
    // grow-only device copies of the caller's host buffers (wepp_place_batch): reads in, results out
    GrowBuf<> io_in, io_out;
    GrowBuf<> pin{true};              // pinned staging of the same (pageable caller buffers go through it)
    std::unique_ptr<HostPool> pool;   // host workers of wepp_place_batch (started by the first large batch)
    // wepp_place_batch as a pipeline: sub-batch k's reads go up on pipe_h2d while the kernels of k-1 run on
    // pipe_compute and the results of k-2 come down on pipe_d2h; one event per sub-batch and stage
    static constexpr uint32_t kPipeMax = 8;
    uint32_t pipe_sub_batches = 0;    // 0: chosen per call (one device call per 2 M reads, at most 8)
    DevStreams<kLanes> pipe_h2d, pipe_d2h, pipe_compute;     // (a set per lane: the two launch threads of a call do not share a stream); made by the first wepp_place_batch
    DevEvents<kPipeMax> pipe_up, pipe_done;
    DevEvents<4 * kPipeMax> pipe_out;   // (one per sub-batch and result array)
    GrowBuf<> pin_out{true};          // pinned staging of the results (the reads' staging is `pin`)
    // plan id of every read of the most recent placement call (k_route writes it; wepp_mat_last_tiers / _plans read it);
    // grow-only, outside the workspace so that the sub-batches of one host call add up to the whole call's picture
    GrowBuf<uint32_t> d_wsid_of;      // window crown (index into DevMAT::wc_info) of the reads routed to slot WC_SLOT, same sizing
    GrowBuf<uint8_t> d_plan_of;
    PlaceLane lane[2];
    static constexpr uint32_t kRing = 64;
    DevEvents<kRing> ev0, ev1;
    std::atomic<uint32_t> ww_by_jobs{0};  // the previous call held too many reads with 17 - 256 events for a wave each: this call cuts their walks into jobs (a hint, like job_events)
    std::atomic<uint32_t> step_walkers{0};  // plain walkers of up to 8 entries of the previous call: above STEP_GROUPS_MAX_WALKERS this call's k_step places them lane = read, not by lane groups (a hint)
    std::atomic<uint32_t> expect_jobs8{0};  // the previous call held reads of the 8-entry job class: this call launches the class blind behind k_route, else from the counters (a hint too)
    std::atomic<uint32_t> expect_lists{0};  // the previous call held reads whose launches read the grouped read list: this call launches k_scatter blind behind the counters' copy, else only once the counters ask for it; bit 1: its last blind launch found no consumer (a hint too: capi.cpp)
    std::atomic<uint64_t> n_timed{0}; // placement calls since the last timing reset (a call claims its slot of the event ring when it starts)
    std::mutex stat_mu;               // the counters below: the sub-batches of a pipelined wepp_place_batch finish on two host threads
    uint64_t plan_reads_in = 0;       // reads of the sub-batches of the current call that have been planned
    uint64_t last_passes = 0, last_bytes = 0;
    uint64_t acc_passes = 0, acc_bytes = 0;   // the same summed over the calls since the last timing reset
    uint64_t last_walk_reads = 0;     // reads of the most recent call that walked their own events (k_walk)
    uint32_t last_n_reads = 0;        // reads of the most recent placement call (wepp_mat_last_tiers)
};

namespace wepp {

// `count` elements of device memory that live as long as the handle, counted in its stats
template <typename T>
inline int dev_alloc(wepp_mat* h, size_t count, T** out) {
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return set_error(WEPP_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    h->allocs.push_back(p);
    h->stats.device_bytes += bytes;
    *out = (T*)p;
    return WEPP_OK;
}

// ... holding a copy of `v`
template <typename T>
inline int upload(wepp_mat* h, const std::vector<T>& v, const T** out) {
    T* p = nullptr;
    WEPP_TRY(dev_alloc(h, v.size(), &p));
    if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = p;
    return WEPP_OK;
}

// defined in capi.cpp, used by place_batch.cpp and pass2_capi.cpp too
size_t pad256(size_t b);
int ensure_plan_buffers(wepp_mat_t* mat, uint32_t plan_total);
int place_device(wepp_mat_t* mat, const uint32_t* d_read_off, const uint32_t* d_read_word, uint32_t n_reads,
                 uint32_t* d_best_bfs_j, int32_t* d_score, uint32_t* d_num_best, uint32_t* d_flags, hipStream_t stream,
                 uint32_t plan_base, uint32_t plan_total, uint32_t lane_idx = 0);

}  // namespace wepp
