// resolve.hpp -- residual mutations against a selection of haplotypes (arena::resolve_unaccounted_mutations,
// src/WEPP/arena.cpp:739-892): shared declarations of resolve_kernels.hip and resolve_capi.cpp.
// See DESIGN.md section 4.8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assign.hpp"

namespace wepp {

constexpr uint32_t RES_WAVES = 4;                    // waves per workgroup of k_resolve_tally
constexpr uint32_t RES_CHUNK = 256;                  // relations of one mutation a workgroup of k_resolve_tally takes at a time (not tuned)
constexpr uint32_t RES_MAX_CHUNK_WGS = 64;           // workgroups per mutation at most: they stride over its chunks (not tuned)
constexpr uint32_t RES_MASKED = 0x80000000u;         // rel_read: the read is masked (clear: covered)

// the mark passes: one thread per read walks its entries against the residual mutations inside its window
struct MarkArgs {
    uint32_t R, M;
    // the residual list sorted by position, stably: the caller's order survives within a position
    const uint32_t* res_pos;      // [M]
    const uint32_t* res_word;     // [M]
    const uint32_t* res_idx;      // [M] place in the caller's list
    const uint32_t* read_off;
    const uint32_t* read_word;
    const int32_t* start;
    const int32_t* end;
    const int32_t* degree;
    const uint32_t* order;        // place in (start, end) order -> read
    // count pass (each [R + 1], the last element zeroed by the caller: the scans' totals)
    uint32_t* n_rel;              // relations of read r
    uint32_t* n_words;            // entries of r' (0: untouched)
    uint32_t* touched;            // 1: read r has a relation
    uint32_t* touched_place;      // the same by place in the window order
    // write pass: the exclusive scans of the four
    const unsigned long long* rel_at;
    const unsigned long long* word_at;
    const unsigned long long* compact;     // read -> touched read
    const unsigned long long* place_at;
    uint32_t* out_off;            // [T + 1] the touched reads r' as a read batch
    uint32_t* out_word;
    int32_t* out_start;
    int32_t* out_end;
    int32_t* out_degree;
    uint32_t* out_order;          // [T] the window order of the touched reads
    uint32_t* rel_key;            // [relations] mutation (caller's index), read-major
    uint32_t* rel_val;            // [relations] read | RES_MASKED
    uint32_t* n_covered;          // [M] zeroed
    uint32_t* n_masked;           // [M] zeroed
};

struct TallyArgs {
    uint32_t M, K, Kp;
    const unsigned long long* rel_off;    // [M + 1]
    const uint32_t* rel_read;             // mutation-major, reads ascending
    const unsigned long long* compact;    // read -> touched read
    const int32_t* degree;                // of the touched reads
    const unsigned long long* ties;       // k_assign's, of the touched reads
    uint32_t* hap_reads;                  // [M][K] zeroed
    unsigned long long* hap_degree;       // [M][K] zeroed
};

hipError_t launch_resolve_count(const MarkArgs& a, hipStream_t stream);
hipError_t launch_resolve_write(const MarkArgs& a, hipStream_t stream);
// (key, value) pairs by key, stably: read-major pairs become mutation-major with the reads still ascending
hipError_t resolve_sort_temp_bytes(uint64_t n, uint32_t key_bits, size_t* bytes);
hipError_t launch_resolve_sort(const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                               uint64_t n, uint32_t key_bits, void* temp, size_t temp_bytes, hipStream_t stream);
// rel_off[m] <- first place of the sorted keys that holds m or more, m = 0 .. M
hipError_t launch_resolve_offsets(const uint32_t* keys, uint64_t n, uint32_t M, unsigned long long* rel_off, hipStream_t stream);
// max_chunks: chunks of the longest relation list
hipError_t launch_resolve_tally(const TallyArgs& a, uint64_t max_chunks, hipStream_t stream);
// best_degree[m] <- max of hap_degree over the columns with hap_reads > 0 (0: none); best_mask: those attaining it
hipError_t launch_resolve_best(const uint32_t* hap_reads, const unsigned long long* hap_degree, uint32_t M, uint32_t K,
                               long long* best_degree, uint32_t* best_mask, hipStream_t stream);

}  // namespace wepp
