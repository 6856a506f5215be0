// geno.hpp -- pairwise distances between the genotypes of full-tree nodes (get_mutations + mutation_distance,
// src/WEPP/util.cpp:188-222, 271-296, as dump_haplotype_uncertainty and print_mutation_distance of arena.cpp use
// them): shared declarations of geno_kernels.hip and geno_capi.cpp.  See DESIGN.md section 4.9.
//
// columns: the kept positions of a set (a group, or A and B together) sorted and made unique; every word gets the
//          index of its position among its set's columns
// planes:  per item four bit-planes (one per bit of mut_nuc) of ceil(columns of its set / 64) 64-bit words, zero where
//          the item has no entry.  Layout: planes[set_base + (item_in_set * W + word) * 4 + plane]
// pairs:   d(a, b) = sum over the words of popcll((a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2) | (a3 ^ b3))
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wepp {

// The planes of the groups of one pass take at most GENO_PASS_BYTES of device memory; the groups of a call are worked
// off in passes of consecutive groups.  WEPP_GENO_PASS_BYTES in the environment (diagnostic) lowers the bound; a group
// that exceeds the lowered bound gets a pass of its own, one that exceeds GENO_PASS_BYTES is WEPP_ELIMIT.
constexpr uint64_t GENO_PASS_BYTES = 1ull << 30;
constexpr uint32_t GENO_BLOCK = 256;            // threads per workgroup of every kernel here
constexpr uint32_t GENO_WAVE_ITEMS = 64;        // groups of at most this many items take one wave each (k_geno_wave)
constexpr uint32_t GENO_TILE = 64;              // items per side of a tile of k_geno_tile (one workgroup per tile)
constexpr uint32_t GENO_CHUNK_WORDS = 4;        // 64-bit column words per LDS chunk: 2 tiles x 64 items x 4 words x 4 planes x 8 B = 16 KiB
constexpr uint32_t GENO_TILE_PAD = GENO_TILE + 1;   // LDS row stride of the A tile (items are the fast index; the pad spreads the staging stores over the banks)
constexpr uint32_t GENO_JOBS_PER_LAUNCH = 1u << 20; // tiles per launch of k_geno_tile (the host lists them in chunks)
constexpr uint64_t GENO_MAX_MATRIX_CELLS = 1ull << 28;   // wepp_geno_nearest's optional matrix (1 GiB of int32)
constexpr uint32_t GENO_POS_BITS = 20;          // a sort key is (set << GENO_POS_BITS) | position
constexpr uint32_t GENO_NO_COLUMN = 0xFFFFFFFFu;    // column of a word the keep mask drops

struct GenoWords {                              // the items' words on the device
    unsigned long long n_words;
    uint32_t n_items, n_sets;
    const unsigned long long* item_off;         // [n_items + 1]
    const uint32_t* item_word;
    const uint32_t* set_off;                    // [n_sets + 1] over the items, or null: every item is in set 0
    const uint32_t* keep_bits;                  // or null
    uint32_t keep_positions;
};

// key[i] <- (set << 20) | position of word i, or n_sets << 20 where the keep mask drops it; val[i] <- i
hipError_t launch_geno_keys(const GenoWords& w, unsigned long long* key, uint32_t* val, hipStream_t stream);
// a stable sort of (key, val) by the low key_bits bits
hipError_t geno_sort_temp_bytes(unsigned long long n, uint32_t key_bits, size_t* bytes);
hipError_t launch_geno_sort(const unsigned long long* key_in, unsigned long long* key_out, const uint32_t* val_in, uint32_t* val_out,
                            unsigned long long n, uint32_t key_bits, void* temp, size_t temp_bytes, hipStream_t stream);
// head[j] <- 1 where sorted key j is a kept word's and differs from key j - 1; head[n] <- 0
hipError_t launch_geno_heads(const unsigned long long* key, unsigned long long n, uint32_t n_sets, uint32_t* head, hipStream_t stream);
// exclusive prefix sums of n + 1 32-bit counts (rank[n] = the number of heads)
hipError_t geno_scan_temp_bytes(unsigned long long n, size_t* bytes);
hipError_t launch_geno_scan(const uint32_t* head, uint32_t* rank, unsigned long long n, void* temp, size_t temp_bytes, hipStream_t stream);
// set_first[s] <- the global column of the first column of set s (sets without a kept word are not written),
// set_cols[s] (zeroed by the caller) <- its number of columns
hipError_t launch_geno_sets(const unsigned long long* key, const uint32_t* head, const uint32_t* rank, unsigned long long n, uint32_t n_sets,
                            uint32_t* set_first, uint32_t* set_cols, hipStream_t stream);
// word_col[val[j]] <- the column of the word within its set, GENO_NO_COLUMN for a dropped word
hipError_t launch_geno_word_cols(const unsigned long long* key, const uint32_t* val, const uint32_t* head, const uint32_t* rank,
                                 unsigned long long n, uint32_t n_sets, const uint32_t* set_first, uint32_t* word_col, hipStream_t stream);

struct GenoPass {                               // the sets [set0, set0 + n_sets) of a pass; the tables are indexed by set - set0
    uint32_t set0, n_sets;
    uint32_t item0, n_items;                    // their items
    const unsigned long long* set_base;         // [n_sets] first plane word of the set
    const uint32_t* set_item0;                  // [n_sets] first item of the set
    const uint32_t* set_items;                  // [n_sets] items of the set
    const uint32_t* set_words;                  // [n_sets] W = ceil(columns / 64)
    unsigned long long* planes;
};
// planes (zeroed by the caller) <- the bits of the pass's words [first_word, end_word)
hipError_t launch_geno_planes(const GenoWords& w, const uint32_t* word_col, const GenoPass& p, unsigned long long first_word,
                              unsigned long long end_word, hipStream_t stream);

struct GenoTileJob { uint32_t set, ti, tj; };   // set relative to the pass; tile ti of the rows against tile tj of the columns

// diam[set0 + small[k]] <- max(itself, the largest distance of two items of that set), one wave per listed set (2 .. GENO_WAVE_ITEMS items)
hipError_t launch_geno_wave(const GenoPass& p, const uint32_t* small, uint32_t n_small, int32_t* diam, hipStream_t stream);
// the same for the listed tiles of larger sets (ti <= tj)
hipError_t launch_geno_tile_diam(const GenoPass& p, const GenoTileJob* jobs, uint32_t n_jobs, int32_t* diam, hipStream_t stream);
// set 0 holds A (items [0, n_a)) and B (the rest): best[a] <- min(itself, (d(a, b) << 32) | b) over the b of tile tj,
// matrix[a * n_b + b] <- d(a, b) when matrix is not null
hipError_t launch_geno_tile_nearest(const GenoPass& p, const GenoTileJob* jobs, uint32_t n_jobs, uint32_t n_a, unsigned long long* best,
                                    int32_t* matrix, hipStream_t stream);

}  // namespace wepp
