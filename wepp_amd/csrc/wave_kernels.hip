// wave_kernels.hip -- a read with MANY events at its positions: lane = list entry, one wavefront per 64 entries.
//
// The per-read walk (walk_kernels.hip) visits a read's events one after the other -- a chain of dependent gathers,
// ~1 us each: fine for the reads of a sequencing run (0-16 events), slow for the one read in a thousand that lists a
// frequently mutated position (17 to a few hundred events in its stream).  Round 2 cut such walks into jobs of 8
// events (gather + scan + walk + combine: ~85 us of latency for ~1 000 reads, the longest chain of the default step).
// Here the events of ONE read are spread over the lanes of one wave and nothing is walked:
//   * every lane loads up to WW_R entries of the read's position lists (an entry = a mutation of a stream node at a
//     listed position, with the node's subtree end: flatmat.hpp IxEnt) -- coalesced, the lists are contiguous;
//   * every entry learns what a sequential walk would know on arrival: c_S in front of its node = c_S of an empty path
//     + the deltas of the entries whose subtree holds the node; the other entries of the same node (a node that mutates
//     several listed positions); and, for the two stretches of untouched nodes that start behind an entry -- its
//     descendants, from node + 1, and what follows its subtree, from end --, their c_S, where they stop (the next node,
//     descendant start or subtree end of any entry) and whether another entry owns the same stretch.  Up to 64 entries:
//     an all-pairs pass of register broadcasts on the read's one wave.  More: all of these are ranks, prefix sums and
//     successors over the entries' node and end keys, so the workgroup sorts both key sets in LDS, scans the deltas in
//     both orders and every entry asks six binary searches (place_dev.hpp: sorted_build, sorted_query);
//   * every lane scores its node (the formula of the walk and of the sweep's node-by-node path, usher_mapper.cpp:
//     191-265, 455-456) and asks the range queries of its stretches (one byte of the sparse table, then four 16-byte
//     loads: flatmat.hpp), all lanes at once;
//   * a wave reduction leaves (score, rank, count, has_unique).
// The device code is in place_dev.hpp (wave_walk_body, wave_read): by default it runs in the first workgroups of k_step
// (walk_kernels.hip), in one launch with the plain walks; this unit keeps the launch of its own (WEPP_STEP_UNFUSED=1).
// A read with more than 64 events takes all waves of a workgroup: they sort together, wave r % W scores row r.
// A handful of dependent memory round trips per read, whatever its events.  Exact: the same nodes get the same scores
// as in the sequential walk (tests/walk_model.py is the CPU model of that walk; the GPU parity tests cover this kernel
// through every batch that holds such reads, and test_reads_with_many_events_vs_oracle aims at it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_mat.hpp"
#include "place_dev.hpp"

namespace wepp {

namespace {
constexpr uint32_t WW_WAVES = WW_R;                        // waves of a block: a wave per row of the largest read
constexpr uint32_t WW_WGS = 1024;                         // persistent grid: the waves loop over the list
}  // namespace

// The many-event reads in a launch of their own (WEPP_STEP_UNFUSED=1, and every caller without a plain walk beside
// them); by default the wave-role workgroups of k_step (walk_kernels.hip) run the same body.  The device code is in
// place_dev.hpp: wave_walk_body.
__global__ __launch_bounds__(64 * WW_WAVES) void k_walk_wave(DevMAT m, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count, uint32_t n_reads,
                                                                const uint32_t* __restrict__ read_off, const uint32_t* __restrict__ read_word,
                                                                const int32_t* __restrict__ root_score, uint32_t* __restrict__ best_bfs_j,
                                                                int32_t* __restrict__ score_out, uint32_t* __restrict__ num_best,
                                                                uint32_t* __restrict__ flags, unsigned long long* __restrict__ work_counter,
                                                                const uint32_t* __restrict__ wsid) {
    static_assert(WAVE_WALK_MAX_EVENTS == 64 * WW_WAVES, "a block holds the largest read");
    __shared__ __attribute__((aligned(16))) uint32_t lds[ww_lds_words(WW_WAVES)];      // (64-bit sort keys)
    const uint32_t n_small = (uint32_t)__builtin_amdgcn_readfirstlane((int)count[0]), n_big = (uint32_t)__builtin_amdgcn_readfirstlane((int)count[1]);
    wave_walk_body<WW_WAVES>(m, lds, blockIdx.x, gridDim.x, list, n_small, n_big, n_reads, read_off, read_word, root_score, best_bfs_j, score_out, num_best,
                             flags, work_counter, wsid);
}

hipError_t launch_walk_wave(const DevMAT& m, const uint32_t* list, const uint32_t* count, uint32_t n_reads, const CallReads& rd, const CallResults& out,
                            unsigned long long* work_counter, hipStream_t stream) {
    hipLaunchKernelGGL(k_walk_wave, dim3(WW_WGS), dim3(64 * WW_WAVES), 0, stream, m, list, count, n_reads, rd.off, rd.word, rd.root_score,
                       out.best_bfs_j, out.score, out.num_best, out.flags, work_counter, rd.wsid);
    return hipGetLastError();
}

}  // namespace wepp
