// peaks.hpp -- the peak-removal loop of wepp_filter (step / singular_step / find_correspondents / remove_read /
// clear_neighbors, src/WEPP/initial_filter.cpp:241-453): shared declarations of peaks_kernels.hip and
// peaks_capi.cpp.  See DESIGN.md section 4.8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wepp {

constexpr uint32_t PEAK_BLOCK = 256;       // threads per workgroup of every kernel here
constexpr uint32_t PEAK_MAX_WGS = 2048;    // grid-stride beyond this many workgroups

struct PeakTop {                   // what k_peak_max / k_peak_ties leave for the host (zeroed before every step)
    unsigned long long m_bits;     // the largest full score of a live haplotype, as the bits of a non-negative double
    uint32_t n_live;               // live haplotypes
    uint32_t n_tie;                // live haplotypes within eps of the largest
};

// live = not mapped and score > eps; full = score * sqrt(divergence)
hipError_t launch_peak_max(uint32_t N, const double* score, const double* divergence, const uint8_t* mapped, double eps,
                           PeakTop* top, hipStream_t stream);
// group[0 .. top->n_tie) <- the live haplotypes with m - full < eps (any order), group_full their full scores;
// both hold N entries, which no tie group exceeds
hipError_t launch_peak_ties(uint32_t N, const double* score, const double* divergence, const uint8_t* mapped, double eps,
                            PeakTop* top, uint32_t* group, double* group_full, hipStream_t stream);
// out[i] <- field[group[i]][col] of a distance field of N + 1 rows and Es columns
hipError_t launch_peak_gather(const int32_t* field, uint32_t Es, uint32_t col, uint32_t N, const uint32_t* group, uint32_t n,
                              int32_t* out, hipStream_t stream);
// mapped[nodes[i]] <- 1 (entries that are no arena index are passed over)
hipError_t launch_peak_mark(const uint32_t* nodes, uint64_t n, uint32_t N, uint8_t* mapped, hipStream_t stream);

struct PeakHitsArgs {
    uint32_t R, K, Kp, max_pos;
    const uint8_t* geno;           // the accepted peaks' genotype table (assign.hpp): rows 0 .. max_pos of Kp columns
    const uint16_t* pre;
    const uint32_t* read_off;
    const uint32_t* read_word;
    const int32_t* start;
    const int32_t* end;
    const int32_t* degree;
    const uint32_t* order;         // place in window order -> read
    const int32_t* best;           // [R] per place: the map's max_parsimony
    uint8_t* alive;                // [R] per place: the read is still in the remaining set
    int32_t step;
    uint32_t peak_base;            // place of column 0 in the list of peaks
    int32_t* removed_step;         // [R] per read
    uint32_t* removed_peak;        // [R] per read
    uint32_t* hits;                // [R] places of the reads removed by this launch (any order)
    uint32_t* n_hits;              // zeroed
    uint32_t* peak_reads;          // [peak_base + K ..) tallies of the peaks
    unsigned long long* peak_degree;
};
// one lane per place: the first column k with d(read, k) == best takes the read
hipError_t launch_peak_hits(const PeakHitsArgs& a, hipStream_t stream);
// out[i] <- -q[places[i]]
hipError_t launch_peak_negq(uint32_t n, const uint32_t* places, const long long* q, long long* out, hipStream_t stream);

}  // namespace wepp
