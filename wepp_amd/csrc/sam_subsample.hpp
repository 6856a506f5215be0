// sam_subsample.hpp -- read subsampling in front of sam::build (sam::subsample, src/WEPP/sam2pb.cpp:362-454): shared
// declarations of sam_subsample_kernels.hip and sam_subsample_capi.cpp.  The rule is stated in include/wepp_place.h
// (wepp_sam_build_subsampled) and DESIGN.md section 4.10.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sam.hpp"

namespace wepp {

constexpr uint32_t SUB_MAX_TRIALS = 65536;     // trials of one call
constexpr uint32_t SUB_BATCH = 8;              // B: trials whose tables one workgroup of the trial pile-up fills
constexpr uint32_t SUB_TILE = 256;             // sites per tile of it: B x 256 x 6 counters of 32 bits in LDS (48 KiB)
constexpr uint32_t SUB_SEGMENTS = SUB_TILE / 64;   // rounds of a wave that cover a read's part inside a tile
constexpr uint32_t SUB_PILE_BLOCK = 512;       // threads per workgroup of it: 3 workgroups of 8 waves share a CU's 160 KiB of LDS
constexpr uint32_t SUB_CHUNK = 512;            // smallest chunk of a tile's read list one workgroup works off
constexpr uint32_t SUB_PILE_WGS = 8192;        // workgroups one launch of it aims at
constexpr uint32_t SUB_DIGIT_BITS = 11;        // the radix select's digit: 2048 bins of 32 bits in LDS (8 KiB)
constexpr uint32_t SUB_BINS = 1u << SUB_DIGIT_BITS;
constexpr uint32_t SUB_SELECT_TRIALS = 4096;   // trials whose histograms are in memory at once (32 MiB)
// The tables of the trials of one pass take at most SUB_PASS_BYTES of device memory (a pass holds whole batches, at
// least one: 8 tables of 2^20 sites are 192 MiB); the trials of a call are worked off in passes of consecutive
// trials.  WEPP_SAM_SUBSAMPLE_PASS_BYTES in the environment (diagnostic, read once per call) lowers the bound.
constexpr uint64_t SUB_PASS_BYTES = 256ull << 20;

__host__ __device__ inline unsigned long long sub_hash(unsigned long long x) {       // the splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// ---- thresholds: a radix select over keys computed on the fly, most significant digit first -----------------------
// pass p looks at the digit of `width` bits at `shift`; a key takes part when its bits above the digit equal prefix[t]
// hist[n_trials * SUB_BINS] (zeroed) += the digits of the keys of trials [0, n_trials) (trial_hash per trial)
hipError_t launch_sub_histogram(const unsigned long long* trial_hash, const unsigned long long* prefix, uint32_t n_trials, uint32_t n_reads,
                                uint32_t shift, uint32_t width, bool first, uint32_t* hist, hipStream_t stream);
// per trial: the bin that holds the key of rank[t] (0-based among the keys that took part) goes into prefix[t],
// rank[t] becomes the rank inside that bin
hipError_t launch_sub_pick_digit(const uint32_t* hist, uint32_t n_trials, uint32_t width, unsigned long long* prefix, uint32_t* rank, hipStream_t stream);

// ---- trial pile-up ----------------------------------------------------------------------------------------------------
// tile_count[tile] (zeroed) += the reads that meet the tile
hipError_t launch_sub_bin_count(const SamReadsDev& rd, uint32_t* tile_count, hipStream_t stream);
// list[tile_off[tile] ..) <- those reads, in no fixed order (cursor[tiles] zeroed); the sums taken over a list do not depend on it
hipError_t launch_sub_bin_fill(const SamReadsDev& rd, const unsigned long long* tile_off, uint32_t* cursor, uint32_t* list, hipStream_t stream);
// tables[b * G * 6 ..) (zeroed) += the columns, N included, of the reads r with key(t, r) <= thr[t] for the trials
// t = t0 + b, b < n_trials; longest_list = the longest tile list
hipError_t launch_sub_pileup(const SamReadsDev& rd, const unsigned long long* tile_off, const uint32_t* list, uint32_t longest_list,
                             const unsigned long long* trial_hash, const unsigned long long* thr, uint32_t t0, uint32_t n_trials,
                             uint32_t* tables, hipStream_t stream);

// ---- divergence and pick ----------------------------------------------------------------------------------------------
// *covered (zeroed) += the sites of freq with a count
hipError_t launch_sub_covered(const uint32_t* freq, uint32_t G, uint32_t* covered, hipStream_t stream);
// divergence[t0 + b] <- D of tables[b] against freq, one workgroup per trial, a fixed order of summation
hipError_t launch_sub_divergence(const uint32_t* freq, const uint32_t* covered, uint32_t G, const uint32_t* tables, uint32_t t0, uint32_t n_trials,
                                 double* divergence, hipStream_t stream);
// *best <- the trial of the smallest divergence, the lowest among equals
hipError_t launch_sub_argmin(const double* divergence, uint32_t n_trials, uint32_t* best, hipStream_t stream);

// ---- compaction -------------------------------------------------------------------------------------------------------
// flag[r] <- key(*best, r) <= thr[*best]   (flag holds R + 1 entries; the last one is the caller's)
hipError_t launch_sub_flags(uint32_t R, const unsigned long long* trial_hash, const unsigned long long* thr, const uint32_t* best, uint32_t* flag,
                            hipStream_t stream);
// with flag_off = the exclusive scan of flag: kept[j] <- the j-th flagged read, kept_start[j] / kept_len[j] its window
hipError_t launch_sub_kept(const SamReadsDev& rd, const uint32_t* flag, const unsigned long long* flag_off, uint32_t* kept, uint32_t* kept_start,
                           uint32_t* kept_len, hipStream_t stream);
// kept_base[kept_off[j] ..) <- the columns of read kept[j], one wave per read
hipError_t launch_sub_gather(const SamReadsDev& rd, uint32_t n_kept, const uint32_t* kept, const unsigned long long* kept_off, uint8_t* kept_base,
                             hipStream_t stream);

}  // namespace wepp
