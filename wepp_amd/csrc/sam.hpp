// sam.hpp -- aligned reads to merged reads (sam::build, src/WEPP/sam2pb.cpp:262-275, 281-314, 456-470): shared
// declarations of sam_kernels.hip and sam_capi.cpp.  See DESIGN.md section 4.8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wepp {

constexpr uint32_t SAM_BLOCK = 256;        // threads per workgroup of every kernel here
constexpr uint32_t SAM_TILE = 2048;        // sites per pile-up tile: 6 counters of 32 bits each in LDS (48 KiB)
constexpr uint32_t SAM_PILE_WGS = 2048;    // workgroups the pile-up aims at (tiles x chunks of reads)
constexpr uint32_t SAM_CODE_N = 4, SAM_CODE_GAP = 5;   // "ACGTN_"

struct SamReadsDev {                       // the aligned reads on the device
    uint32_t R;
    const uint32_t* start;                 // [R] 0-based
    const unsigned long long* base_off;    // [R + 1]
    const uint8_t* base;
    const uint8_t* ref;                    // [G] the reference's characters
    uint32_t G;
};

// freq[G * 6] (zeroed) += the columns of every read, N columns left out; *bad_base (zeroed) <- 1 when a byte is > 5
hipError_t launch_sam_pileup(const SamReadsDev& rd, uint32_t* freq, uint32_t* bad_base, hipStream_t stream);
// keep[site * 6 + c] <- the code 0..4 a column with code c at the site has after the correction
hipError_t launch_sam_keep(const uint32_t* freq, uint32_t G, double min_af, uint32_t min_depth, uint8_t* keep, hipStream_t stream);
// n_words[r] <- the columns of read r whose corrected character differs from the reference character
hipError_t launch_sam_count(const SamReadsDev& rd, const uint8_t* keep, uint32_t* n_words, hipStream_t stream);
// words[word_off[r] ..) <- those columns' words, ascending by position
hipError_t launch_sam_words(const SamReadsDev& rd, const uint8_t* keep, const unsigned long long* word_off, uint32_t* words,
                            hipStream_t stream);
// exclusive prefix sums of 32-bit counts in 64 bits: out[0 .. n] (n + 1 entries, out[n] = the total)
hipError_t sam_scan_temp_bytes(uint32_t n, size_t* bytes);
hipError_t launch_sam_scan(const uint32_t* in, unsigned long long* out, uint32_t n, void* temp, size_t temp_bytes, hipStream_t stream);

struct SamSortArgs {                       // what the comparator reads
    const uint32_t* start;
    const unsigned long long* base_off;
    const unsigned long long* word_off;    // [R + 1] per input read
    const uint32_t* words;
    const uint8_t* ref;
};
// order[0 .. R) <- the reads by (start, length, corrected string in ASCII order, input index): an exact merge sort of
// the indices under a comparator that walks the two word lists
hipError_t sam_sort_temp_bytes(uint32_t R, size_t* bytes);
hipError_t launch_sam_sort(const SamSortArgs& a, uint32_t R, uint32_t* iota, uint32_t* order, void* temp, size_t temp_bytes, hipStream_t stream);
// head[s] <- 1 when the read at place s differs from the one at place s - 1 (or s == 0)
hipError_t launch_sam_heads(const SamSortArgs& a, uint32_t R, const uint32_t* order, uint32_t* head, hipStream_t stream);
// with head_off = the exclusive scan of head (R + 1 entries): group_off[g] <- the place of the g-th head,
// group_off[n_merged] <- R, and lead_words[g] <- the word count of the read at that place
hipError_t launch_sam_groups(uint32_t R, const uint32_t* order, const uint32_t* head, const unsigned long long* head_off,
                             const unsigned long long* word_off, uint32_t* group_off, uint32_t* lead_words, hipStream_t stream);
struct SamMergedDev {                      // the merged batch on the device (the fields of wepp_epp_reads)
    uint32_t* read_off;                    // [n_merged + 1]
    uint32_t* read_word;
    int32_t *start, *end, *degree;
};
// one wave per merged read: its window, its degree and the words of its leader (merged_off = the scan of lead_words)
hipError_t launch_sam_merge(const SamSortArgs& a, uint32_t n_merged, const uint32_t* order, const uint32_t* group_off,
                            const unsigned long long* merged_off, const SamMergedDev& out, hipStream_t stream);

}  // namespace wepp
