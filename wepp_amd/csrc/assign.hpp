// assign.hpp -- reads against a SELECTION of haplotypes (arena::dump_read2haplotype_mapping,
// src/WEPP/arena.cpp:590-696): shared declarations of assign_kernels.hip and assign_capi.cpp.
// See DESIGN.md section 4.8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wepp {

// layout units of k_assign: a lane owns ASG_LANE_HAPS consecutive columns of the genotype table, a wave
// therefore a SLAB of 256; the distances of ASG_REG_SLABS slabs stay in registers between the minimum and
// the look for the ties (selections beyond 1024 haplotypes compute theirs twice)
constexpr uint32_t ASG_LANE_HAPS = 4;
constexpr uint32_t ASG_SLAB = 64 * ASG_LANE_HAPS;
constexpr uint32_t ASG_REG_SLABS = 4;
constexpr uint32_t ASG_WAVES = 4;                    // waves per workgroup of k_assign (they share its LDS counters)
constexpr uint32_t ASG_MAX_WGS = 2048;               // persistent grid: the waves stride over the reads
constexpr uint32_t ASG_LDS_MAX_COLS = 5120;          // columns up to which a workgroup aggregates sel_reads / sel_degree in LDS (12 B each)
constexpr uint32_t ASG_SCAN_ROWS = 256;              // rows per block of the prefix-count scan
constexpr uint64_t ASG_MAX_TABLE_BYTES = 1ull << 30; // geno + pre of one call
constexpr uint32_t ASG_MAX_PRE = 65535;              // 16-bit prefix counts

inline uint32_t assign_padded_cols(uint32_t n_sel) { return (n_sel + ASG_SLAB - 1) / ASG_SLAB * ASG_SLAB; }

struct AssignArgs {
    uint32_t R, K, Kp, max_pos, genome_size, cover_words;
    // the selection's genotype table, position-major: rows 0 .. max_pos of Kp columns
    const uint8_t* geno;          // allele mask, 0 = reference
    const uint16_t* pre;          // non-reference positions <= the row's
    const uint32_t* read_off;
    const uint32_t* read_word;
    const int32_t* start;
    const int32_t* end;
    const int32_t* degree;
    const uint32_t* order;        // place in (start, end) order -> read
    int32_t* min_dist;            // [R]
    uint32_t* n_epp;              // [R]
    unsigned long long* ties;     // [R][Kp / 256][4] lanes whose j-th column attains the minimum, or nullptr (no lists wanted)
    uint32_t* sel_reads;          // [Kp] zeroed
    unsigned long long* sel_degree;   // [Kp] zeroed
    uint32_t* cover;              // [K][cover_words] zeroed
};

// geno (zeroed by the caller) <- the genotypes of sel[0 .. K), marker bit 0x80 on every cell a mutation
// of the root path has claimed; then the marker is stripped and pre is filled.  block_sums: [ceil((max_pos + 1) /
// ASG_SCAN_ROWS)][Kp] uint32; *overflow (zeroed by the caller) receives the largest count of a column.
hipError_t launch_assign_tables(const uint32_t* node_woff, const uint32_t* words, const uint32_t* parent_dfs,
                                const uint32_t* sel, uint32_t K, uint32_t Kp, uint32_t max_pos, uint8_t* geno,
                                uint16_t* pre, uint32_t* block_sums, uint32_t* overflow, hipStream_t stream);
hipError_t launch_assign(const AssignArgs& a, hipStream_t stream);
// asg_off[0 .. R] <- exclusive scan of n_epp (64-bit sums)
hipError_t assign_scan_temp_bytes(uint32_t R, size_t* bytes);
hipError_t launch_assign_scan(const uint32_t* n_epp, unsigned long long* asg_off, uint32_t R, void* temp,
                              size_t temp_bytes, hipStream_t stream);
// asg_sel[asg_off[r] ..) <- the indices into sel attaining read r's minimum, ascending
hipError_t launch_assign_lists(const unsigned long long* ties, const unsigned long long* asg_off, uint32_t R,
                               uint32_t Kp, uint32_t* asg_sel, hipStream_t stream);
// sel_covered[k] <- set bits of row k of the coverage bitmap
hipError_t launch_assign_popcount(const uint32_t* cover, uint32_t K, uint32_t cover_words, uint32_t* sel_covered,
                                  hipStream_t stream);

}  // namespace wepp
