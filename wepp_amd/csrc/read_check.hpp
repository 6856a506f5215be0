// read_check.hpp -- the pure host logic of a batch that comes in host buffers (wepp_place_batch, place_batch.cpp; the
// pass-2 calls, pass2_capi.cpp): the checks of a read CSR, the cut of a batch into sub-batches, copy chunks and staging
// parts, and which task stages / which copy sends which offset.  No device, no threads: tests/cxx/read_check_main.cpp
// includes this header alone and runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/wepp_place.h"
#include "errors.hpp"

namespace wepp {

// shared argument check of the calls that take a read CSR from the host: offsets start at 0, are monotone and
// stay inside the word array (whose size is read_off[n_reads])
inline int check_read_csr(const uint32_t* read_off, const uint32_t* read_word, uint32_t n_reads) {
    if (!read_off) return set_error(WEPP_EINVAL, "null read_off");
    if (read_off[0] != 0) return set_error(WEPP_EINVAL, "read_off[0] must be 0");
    for (uint32_t r = 0; r < n_reads; r++)
        if (read_off[r + 1] < read_off[r]) return set_error(WEPP_EINVAL, "read_off not monotone");
    if (read_off[n_reads] && !read_word) return set_error(WEPP_EINVAL, "null read_word");
    return WEPP_OK;
}

// ---- the range check ----
// preconditions of the reference's merge (usher_mapper.cpp:205-243): sorted, unique positions.  The first offending
// read of [lo, hi) goes to `bad`, its kind to `what`: 0 offsets, 1 order or uniqueness of the positions, 2 a zero
// nucleotide mask.  Both are left alone when the range is clean.  `nw` is the size of the word array.

// exact, read by read: only run on a range the fast pass below found something in
inline void check_reads_exact(const uint32_t* read_off, const uint32_t* read_word, uint64_t nw, uint32_t lo, uint32_t hi,
                              uint32_t& bad, int& what) {
    for (uint32_t r = lo; r < hi; r++) {
        if (read_off[r + 1] < read_off[r] || read_off[r + 1] > nw) { bad = r; what = 0; return; }
        for (uint32_t k = read_off[r] + 1; k < read_off[r + 1]; k++)
            if ((read_word[k] & 0xFFFFFu) <= (read_word[k - 1] & 0xFFFFFu)) { bad = r; what = 1; return; }
        for (uint32_t k = read_off[r]; k < read_off[r + 1]; k++)
            if (((read_word[k] >> 24) & 15u) == 0 || ((read_word[k] >> 20) & 15u) == 0) { bad = r; what = 2; return; }
    }
}

// fast pass over a range of reads: branch-free loops the compiler vectorises.  Offsets: monotone and inside
// the word array.  Words: no zero mask; positions ascend from one word to the next except where a read
// starts -- the descents are counted over all words and over the read starts, and must be the same number.
// With `stage_word` the words of the range are moved into the staging buffer as they are looked at (one pass over
// the input); nothing is moved when the offsets of the range are not valid.
inline void check_reads(const uint32_t* read_off, const uint32_t* read_word, uint64_t nw, uint32_t lo, uint32_t hi,
                        uint32_t* stage_word, uint32_t& bad, int& what) {
    uint32_t off_bad = (read_off[lo] > nw) ? 1u : 0u;
    for (uint32_t r = lo; r < hi; r++) {
        const uint32_t a = read_off[r], b = read_off[r + 1];
        off_bad |= (uint32_t)(b < a) | (uint32_t)(b > nw);
    }
    if (off_bad) { check_reads_exact(read_off, read_word, nw, lo, hi, bad, what); return; }
    const uint32_t a0 = read_off[lo], b0 = read_off[hi];
    uint32_t zero = 0, descents = 0, at_starts = 0;
    if (stage_word) {
        for (uint32_t k = a0; k < b0; k++) {
            const uint32_t w = read_word[k];
            zero |= (uint32_t)(((w >> 24) & 15u) == 0) | (uint32_t)(((w >> 20) & 15u) == 0);
            stage_word[k] = w;
        }
    } else {
        for (uint32_t k = a0; k < b0; k++) {
            const uint32_t w = read_word[k];
            zero |= (uint32_t)(((w >> 24) & 15u) == 0) | (uint32_t)(((w >> 20) & 15u) == 0);
        }
    }
    for (uint32_t k = a0 + 1; k < b0; k++) descents += (uint32_t)((read_word[k] & 0xFFFFFu) <= (read_word[k - 1] & 0xFFFFFu));
    for (uint32_t r = lo + 1; r < hi; r++) {
        const uint32_t s0 = read_off[r];
        if (read_off[r + 1] > s0 && s0 > a0) at_starts += (uint32_t)((read_word[s0] & 0xFFFFFu) <= (read_word[s0 - 1] & 0xFFFFFu));
    }
    if (zero || descents != at_starts) check_reads_exact(read_off, read_word, nw, lo, hi, bad, what);
}

// ---- the batch geometry ----
constexpr uint32_t BIG_BATCH_READS = 1u << 16;   // from here on a batch is checked, staged and moved out by the handle's host workers
constexpr uint32_t PIPE_MAX_SUB_BATCHES = 8;     // (wepp_mat::kPipeMax)

struct BatchGeometry {
    uint32_t n_reads = 0;
    bool big = false;            // the host workers take part
    bool two_launchers = false;  // even sub-batches are launched by the calling thread, odd ones by a worker
    uint32_t S = 1;              // sub-batches = device calls
    uint32_t C = 1;              // copy chunks (a multiple of S)
    uint32_t CPS = 1;            // chunks per sub-batch
    uint32_t PS = 1;             // staging parts per chunk
    uint32_t PO = 1;             // copy-out parts per (sub-batch, array)
    uint32_t chunk_lo(uint32_t c) const { return (uint32_t)((uint64_t)n_reads * c / C); }   // first read of chunk c
    uint32_t sub_lo(uint32_t k) const { return chunk_lo(k * CPS); }                         // first read of sub-batch k
};

// `pipe_knob`: wepp_mat_set_pipeline (0: not set), `pipe_env`: WEPP_PIPE_SUBBATCHES (0: not set), `workers`: the threads
// of the handle's pool, `min_chunks`: WEPP_PIPE_MIN_CHUNKS.
// S sub-batches = device calls.  A device call is a chain of ~20 short launches with a host round trip in the
// middle (routing counters): ~0.3 ms whatever its size up to a million short reads, most of it the HOST's share,
// which two calls cannot overlap -- so a batch is only cut into several calls when each keeps >= 2 M reads
// (measured, profiles/r3_experiments/pcie_pipeline.txt: 1 M reads in 2 / 4 / 8 calls 1.41 / 1.98 / 3.07 ms against
// 1.28 in one).  C copy chunks >= S: the reads are checked, staged and sent up chunk by chunk, whatever S.
// (round 4: with two launch threads a call of half a million reads or more goes as two halves, 1.08 -> 1.00 ms per
// 1 M reads; three or four are slower again: the host's HIP calls per device call are what runs out)
inline BatchGeometry batch_geometry(uint32_t n_reads, uint32_t pipe_knob, uint32_t pipe_env, uint32_t workers,
                                    bool per_node_scores, uint32_t min_chunks) {
    BatchGeometry g;
    g.n_reads = n_reads;
    g.big = n_reads >= BIG_BATCH_READS;
    if (!pipe_knob) pipe_knob = pipe_env;
    const bool can_pair = g.big && workers >= 2;
    g.S = !g.big || per_node_scores ? 1u : pipe_knob ? pipe_knob : std::max<uint32_t>((can_pair && n_reads >= (1u << 19)) ? 2u : 1u, n_reads >> 21);
    g.S = std::min<uint32_t>(g.S, PIPE_MAX_SUB_BATCHES);
    g.C = g.big ? g.S * ((min_chunks + g.S - 1) / g.S) : 1;               // (a multiple of S, >= 4 unless WEPP_PIPE_MIN_CHUNKS says otherwise)
    g.CPS = g.C / g.S;
    const uint32_t threads = g.big ? workers + 1 : 1;
    g.PS = g.big ? std::max(1u, (4 * threads + g.C - 1) / g.C) : 1;
    g.PO = g.big ? 4 : 1;
    g.two_launchers = g.big && g.S > 1 && workers >= 2;
    return g;
}

// ---- who stages what ----
// Staging task (chunk ck, part) checks the reads [read_lo, read_hi) and copies the offsets [off_lo, off_hi): its
// reads', and -- the LAST part of a chunk -- the chunk's end offset too: a chunk's H2D copy takes the offsets
// [first read, last read + 1] and is enqueued as soon as the chunk's OWN tasks are done.  (Round 3 left the end offset
// to the first task of the NEXT chunk, which the launch thread does not wait for: with few host workers the copy went
// up before it was staged -- a stale or uninitialised offset for the read at every chunk boundary, wrong entries for
// that read or a fault in k_route.)  The first part of a later chunk leaves its first offset to the chunk before:
// every element has one writer.
struct StageRange { uint32_t read_lo, read_hi, off_lo, off_hi; };

inline StageRange stage_range(const BatchGeometry& g, uint32_t ck, uint32_t part) {
    const uint32_t lo = g.chunk_lo(ck), hi = g.chunk_lo(ck + 1);
    const uint32_t a = lo + (uint32_t)((uint64_t)(hi - lo) * part / g.PS), b = lo + (uint32_t)((uint64_t)(hi - lo) * (part + 1) / g.PS);
    const uint32_t ca = (part == 0 && ck > 0) ? a + 1 : a, cb = (part + 1 == g.PS) ? b + 1 : b;
    return StageRange{a, b, ca, cb};
}

// ---- what a chunk's upload sends and waits for ----
// The H2D copy of chunk ck of sub-batch k sends the offsets [off_lo, off_hi) once every staging task of the chunks
// [wait_lo, ck] is done.  Offset chunk_lo(ck) went up with the chunk before (the kernels of the sub-batch before may be
// reading it) -- but the first chunk of a SUB-BATCH sends its own too: the chunk before belongs to the other launcher,
// whose copy may not be enqueued yet (the same four bytes written twice).  That offset is staged with the chunk
// before it, so the first chunk of a sub-batch waits for that chunk as well.
struct UploadRange { uint32_t off_lo, off_hi, wait_lo; };

inline UploadRange upload_range(const BatchGeometry& g, uint32_t k, uint32_t ck) {
    const uint32_t clo = g.chunk_lo(ck), chi = g.chunk_lo(ck + 1);
    const bool first_of_sub = ck == k * g.CPS;
    return UploadRange{(ck && !first_of_sub) ? clo + 1 : clo, chi + 1, (first_of_sub && ck > 0) ? ck - 1 : ck};
}

}  // namespace wepp
