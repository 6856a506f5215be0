// clades.hpp -- clade assignment of placed samples (usher_common.cpp:597-616): shared declarations of
// clades_kernels.hip and clades_capi.cpp.  See DESIGN.md section 4.12.
//
// A PAIR is a read and one of its optimal nodes (wepp_best_nodes); pair p of read r sits at best_off[r] + k.  A SEGMENT
// is the pairs of one read in one annotation column; its keys (clade ids) are sorted ascending and run-length encoded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_mat.hpp"

namespace wepp {

constexpr uint32_t CLADE_MAX_COLUMNS = 8;
// segments of up to CLADE_WAVE_MAX keys are sorted by one wave in registers, up to CLADE_BLOCK_MAX by one workgroup in
// LDS (4 KiB), longer ones together by one device radix sort over (segment, clade) keys; a segment of one key is its
// own sorted form
constexpr uint32_t CLADE_WAVE_MAX = 64;
constexpr uint32_t CLADE_BLOCK_MAX = 1024;
constexpr uint32_t CLADE_BLOCK_THREADS = 256;

struct CladeArgs {
    uint32_t R, C;                       // reads, annotation columns
    uint32_t P;                          // pairs of all reads (< 2^32 / C)
    const uint32_t* read_off;            // [R + 1]
    const uint32_t* read_word;
    const uint32_t* best_bfs_j;          // [R]
    const uint32_t* best_off;            // [R + 1] CSR of the pairs (32 bits on the device)
    const uint32_t* best_nodes;          // [P] BFS indices, checked by the host
    // [C][2][N] nearest annotated ancestor of the node with DFS index d: [c][0] excluding the node, [c][1] including it
    const uint32_t* tab;
    uint32_t* pair_read;                 // [P] read of every pair
    uint32_t* keys;                      // [C][P] clade of every pair
    uint32_t* sorted;                    // [C][P] the same, every segment ascending
    uint32_t* best_clade;                // [C][R]
    uint32_t* found;                     // [R] zeroed: 1 when best_bfs_j[r] is among read r's nodes
};

// keys / pair_read / best_clade / found; segments of one key also go to `sorted`
hipError_t launch_clade_pairs(const DevMAT& m, const CladeArgs& a, hipStream_t stream);
// the segments of the reads list[0 .. n) in all columns, one wave / one workgroup per segment
hipError_t launch_clade_sort_wave(const CladeArgs& a, const uint32_t* list, uint32_t n, hipStream_t stream);
hipError_t launch_clade_sort_block(const CladeArgs& a, const uint32_t* list, uint32_t n, hipStream_t stream);
// the long segments: reads list[0 .. n) with long_off[n + 1] the prefix sums of their pair counts; key64 / key64_out
// hold C * long_off[n] keys each, segment index in the bits from 32 up
hipError_t clade_sort_long_temp_bytes(uint64_t n_keys, uint32_t end_bit, size_t* bytes);
hipError_t launch_clade_sort_long(const CladeArgs& a, const uint32_t* list, const uint32_t* long_off, uint32_t n,
                                  uint32_t n_long_pairs, unsigned long long* key64, unsigned long long* key64_out,
                                  uint32_t end_bit, void* temp, size_t temp_bytes, hipStream_t stream);
// run-length encoding of `sorted`: head[i] = 1 where a run starts, run_of = its exclusive scan (run_of[C * P] = runs in
// all), then hist_off[C * R + 1], run_start[runs + 1] and hist_clade / hist_count
hipError_t clade_scan_temp_bytes(uint64_t n, size_t* bytes);
hipError_t launch_clade_heads(const CladeArgs& a, uint32_t* head, uint32_t* run_of, unsigned long long* hist_off,
                              void* temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_clade_runs(const CladeArgs& a, const uint32_t* head, const uint32_t* run_of, uint32_t n_runs,
                             uint32_t* run_start, uint32_t* hist_clade, uint32_t* hist_count, hipStream_t stream);

}  // namespace wepp
