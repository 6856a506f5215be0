// epp_host.hpp -- what the host sides of the WEPP entry points (epp_capi.cpp, assign_capi.cpp, resolve_capi.cpp,
// neighbors_capi.cpp) share, each written once and defined in epp_host.cpp: the per-call device blocks and events, a
// wepp_epp_reads batch (validation, window order, device copy), the checks and the genotype table of a selection.
// Nothing here or in assign / resolve / neighbors_capi.cpp knows whether HIP is the device's: tests/epp_emu.py compiles
// them unchanged against emulated kernels and an emulated runtime (tests/cxx/hip_emu), which tests their logic, buffer
// sizes and launch order without a GPU -- not speed, occupancy, the device memory model or asynchrony between streams.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "assign.hpp"
#include "epp.hpp"
#include "handle.hpp"

namespace wepp {

struct DevPool {                       // device allocations of one call, taken from / returned to the handle's cache
    wepp_mat::DevBlockCache& cache;
    std::vector<DevBlock> used;
    explicit DevPool(wepp_mat::DevBlockCache& c) : cache(c) {}
    ~DevPool() {
        (void)hipDeviceSynchronize();  // (a call that fails half-way may still have kernels in flight on these blocks)
        for (auto& b : used) cache.blocks.push_back(b);
    }
    template <typename T>
    hipError_t get(T** out, size_t n) {
        const size_t asked = n * sizeof(T), bytes = (std::max<size_t>(asked, 64) + 255) & ~(size_t)255;
        // the smallest cached block that holds the request without wasting more than half of itself
        size_t best = SIZE_MAX;
        auto& blocks = cache.blocks;
        for (size_t i = 0; i < blocks.size(); i++) {
            const size_t sz = blocks[i].bytes;
            if (sz >= bytes && sz <= 2 * bytes + (1u << 20) && (best == SIZE_MAX || sz < blocks[best].bytes)) best = i;
        }
        if (best != SIZE_MAX) {
            used.push_back(blocks[best]);
            blocks.erase(blocks.begin() + (std::ptrdiff_t)best);
            used.back().asked = std::max(used.back().asked, asked);
            *out = (T*)used.back().ptr;
            return hipSuccess;
        }
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess && !blocks.empty()) {
            // out of memory with blocks of other sizes parked in the cache: release them and try again
            for (auto& b : blocks) (void)hipFree(b.ptr);
            blocks.clear();
            e = hipMalloc(&p, bytes);
        }
        if (e == hipSuccess) used.push_back(DevBlock{p, bytes, asked});
        *out = (T*)p;
        return e;
    }
};

#define DEV_GET(pool, p, n) /* p = n elements from the pool, or the caller returns WEPP_ENOMEM */ \
    do { if (hipError_t _e = (pool).get(&(p), (n))) return set_error(WEPP_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(_e)); } while (0)

// (the events of a call: DevEvents of handle.hpp)

// the reference's preconditions on a read batch, made explicit (read_off / start / end / degree are non-null when n_reads > 0,
// read_word when there are words): WEPP_OK, or WEPP_EINVAL with the message set.  *total_degree receives the sum of the degrees.
int epp_validate_reads(const wepp_epp_reads* rd, long long* total_degree);
// order[s] = the read at place s of the (start, end, index) order: two stable counting passes when the
// window bounds are genome positions, a comparison sort otherwise
void epp_window_order(const wepp_epp_reads* rd, std::vector<uint32_t>& order);

struct DevReads {                      // a read batch on the device
    uint32_t R = 0; uint64_t W = 0;    // reads, words of all reads
    uint32_t *read_off = nullptr, *read_word = nullptr, *order = nullptr;
    int32_t *start = nullptr, *end = nullptr, *degree = nullptr;
};
int alloc_reads(DevPool& pool, uint32_t R, uint64_t W, DevReads* reads);   // the six blocks of R reads with W words: WEPP_OK or WEPP_ENOMEM
int upload_reads(DevPool& pool, const wepp_epp_reads* rd, const std::vector<uint32_t>& order, hipStream_t stream, DevReads* reads);   // ... filled with rd (n_reads > 0) in `order`

// ---- the map's sweep as a routine (epp_sweep.cpp: it launches the kernels of epp_kernels.hip, which the emulated
// library of tests/epp_emu.py does not have, so it stays out of epp_host.cpp) ------------------------------------------
// A planned sweep of the reads order[0 .. n) between its two passes: wepp_epp_map runs it over a whole batch,
// wepp_epp_peaks once more over every subset of reads it takes out of the scores.
struct EppSweep {
    EppSweepArgs a{};                  // groups, streams, partial rows; best / mult / delta_fx per place in `order`
    uint32_t rpl = 1, lds_bytes = 0, tiles_per_group = 1;
    uint64_t events_swept = 0, stream_events = 0;
};
// Plans tiles, groups and jobs for the reads order[..] (in window order; `reads` holds the batch on the device with
// reads.order = the same list), cuts the window streams, runs pass 1 and the combine: a.best / a.mult / a.delta_fx are
// on the device afterwards, delta_fx = round(node_score * fx_scale).  `begin` / `selected` (may be null) are recorded
// before the selection and behind it.  WEPP_OK, WEPP_ELIMIT, WEPP_ENOMEM or WEPP_EDEVICE.
int epp_sweep_pass1(wepp_mat_t* mat, DevPool& pool, const wepp_epp_reads* rd, const std::vector<uint32_t>& order, const DevReads& reads,
                    uint32_t genome_size, double fx_scale, hipStream_t stream, hipEvent_t begin, hipEvent_t selected, EppSweep* sw);
// Pass 2: every node range on which a read attains its minimum receives +delta_fx .. -delta_fx of that read in
// diff_score[N + 1] (delta_fx per place in `order`; null = the combine's own), its degree in diff_cnt (or null), and
// the nodes go to epp_nodes for the reads r with epp_base[r] != ~0 (epp_base is indexed by read).
int epp_sweep_pass2(const EppSweep& sw, const long long* delta_fx, const uint64_t* epp_base, uint32_t* epp_nodes,
                    unsigned long long* diff_score, int* diff_cnt, hipStream_t stream);

// What wepp_epp_map leaves on the device (in the blocks of the caller's pool) for a caller that goes on from it.
struct EppMapState {
    std::vector<uint32_t> order;       // place in window order -> read
    DevReads reads;
    EppSweep sweep;                    // sweep.a.best / mult / delta_fx: P, M and q per place in `order`
    double fx_scale = 1.0;
    unsigned long long* diff_score = nullptr;   // [N + 1] the fixed-point difference array of the scores
    double* score = nullptr;           // [N]
    double* divergence = nullptr;      // [N], when asked for
    void* scan_scratch = nullptr;      // epp_finish_scratch_bytes(N)
    float select_ms = 0, sweep1_ms = 0, sweep2_ms = 0, finish_ms = 0;
    uint32_t groups = 0, jobs = 0;
};
// The body of wepp_epp_map behind its argument checks (n_reads > 0, reads validated, total_degree their degrees' sum):
// every output of `out` is delivered as wepp_epp_map documents it.  want_divergence computes st->divergence even when
// out->hap_divergence is null.
int epp_map_run(wepp_mat_t* mat, DevPool& pool, const wepp_epp_reads* rd, uint32_t genome_size, uint32_t max_cached_epp,
                long long total_degree, wepp_epp_out* out, bool want_divergence, EppMapState* st);

// wepp_epp_neighbors' per-handle preparation (dfs_end on the device, the forced pass size), made by the first call
int nbr_prepare_handle(wepp_mat_t* mat);

// The argument checks of the entry points that take a selection, in the order they are made: what can be said about the
// selection without the handle; the handle, the range of the indices and the read arrays; then (after the entry point has looked at its
// own outputs) genome_size, the read words and the reads' preconditions.  WEPP_OK, or the code with the message set.  `out` is only compared with null.
int assign_check_selection(const wepp_epp_reads* rd, const void* out, uint32_t n_sel, const uint32_t* sel);
int assign_check_handle(const wepp_mat_t* mat, const wepp_epp_reads* rd, uint32_t n_sel, const uint32_t* sel);
int assign_check_reads(const wepp_epp_reads* rd, uint32_t genome_size);
// their two scans, shared with the pivots of neighbors_capi.cpp: "<name>[k] = .. is not an arena index ..", "haplotype .. is <twice>"
int check_arena_indices(const char* name, uint32_t n, const uint32_t* idx, uint32_t N);
int check_distinct(uint32_t n, const uint32_t* idx, const char* twice);

// the selection's genotype table on the device (launch_assign_tables), its blocks taken from `pool`
struct AssignTable {
    uint32_t Kp = 0, max_pos = 0;
    uint8_t* geno = nullptr;
    uint16_t* pre = nullptr;
};
// Checks the table limits, uploads sel, builds the table and waits for it; `begin` / `end` are recorded around
// the device work.  WEPP_OK, WEPP_ELIMIT (table size, 16-bit prefix counts), WEPP_ENOMEM or WEPP_EDEVICE.
int assign_build_table(wepp_mat_t* mat, DevPool& pool, uint32_t n_sel, const uint32_t* sel, hipStream_t stream,
                       hipEvent_t begin, hipEvent_t end, AssignTable* table);

// k_assign's arguments for `reads` against the table of K haplotypes: genome_size, cover_words and the outputs stay the caller's
inline AssignArgs assign_args(const AssignTable& tab, uint32_t K, const DevReads& reads) {
    AssignArgs a{};
    a.R = reads.R; a.K = K; a.Kp = tab.Kp; a.max_pos = tab.max_pos; a.geno = tab.geno; a.pre = tab.pre;
    a.read_off = reads.read_off; a.read_word = reads.read_word; a.start = reads.start; a.end = reads.end; a.degree = reads.degree; a.order = reads.order;
    return a;
}

}  // namespace wepp
