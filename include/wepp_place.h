/*
 * wepp_place.h -- C-ABI of the MI355X read-placement engine.
 *
 * Drop-in boundary for the reference's per-sample node loop.  The reference
 * (TurakhiaLab/WEPP, vendored UShER sources) has no FFI layer; its seam is the
 * C++ call
 *     void mapper2_body(mapper2_input&, bool, bool)          src/usher_graph.hpp:104
 * invoked from the tbb::parallel_for bodies of
 *     int usher_common(...)                                  src/usher_common.hpp:18-22
 *                                                            src/usher_common.cpp:386-411 (pass 1)
 *                                                            src/usher_common.cpp:413-446 (pass 2)
 * This library replaces BOTH passes for a whole batch of samples/reads with one
 * call (wepp_place_batch); INTEGRATION.md shows the few lines a maintainer adds
 * to usher_common.cpp to bind it.
 *
 * Conventions
 *  - plain pointers and sizes only; the caller owns every host buffer;
 *  - every function returns 0 on success or a WEPP_E* code; the message is
 *    available from wepp_last_error() (thread-local).  Nothing here calls
 *    exit() or throws across the boundary (the reference's MAT layer exit(1)s,
 *    src/mutation_annotated_tree.cpp:474,514,533);
 *  - nucleotides are the reference's 4-bit one-hot/IUPAC masks A=1 C=2 G=4 T=8,
 *    N=15 (src/mutation_annotated_tree.cpp:19-74);
 *  - a handle is bound to one device and is not re-entrant: its workspace, routing
 *    counters and staging buffers belong to one call at a time, so the calls on one
 *    handle must be serial AND, for wepp_place_batch_device, ordered on ONE stream
 *    (or separated by a synchronisation).  Different handles -- on different GPUs or
 *    on the same one -- may be used concurrently from different host threads
 *    (tests/test_gpu_parity.py::test_two_handles_two_host_threads).
 */
#ifndef WEPP_PLACE_H
#define WEPP_PLACE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WEPP_OK          0
#define WEPP_EINVAL      1   /* malformed argument / precondition violated      */
#define WEPP_ENOMEM      2   /* host or device allocation failed                */
#define WEPP_EDEVICE     3   /* HIP runtime error (no device, launch failure..) */
#define WEPP_ELIMIT      4   /* input exceeds a documented limit                */

/* ---- packed 32-bit words ---------------------------------------------- *
 * Sample/read entry = one element of Missing_Sample::mutations
 * (src/usher_graph.hpp:34-54, filled by src/mutation_annotated_tree.cpp:2086-2127):
 *     bits  0..19  position (0 .. 2^20-2)
 *     bits 20..23  ref_nuc mask
 *     bits 24..27  mut_nuc mask (15 for N)
 *     bit  28      is_missing
 */
#define WEPP_MAX_POSITION 0xFFFFEu
static inline uint32_t wepp_pack_read_word(uint32_t position, uint32_t ref_nuc, uint32_t mut_nuc,
                                           uint32_t is_missing) {
    return (position & 0xFFFFFu) | ((ref_nuc & 15u) << 20) | ((mut_nuc & 15u) << 24) |
           ((is_missing & 1u) << 28);
}

/* ---- the tree as the caller hands it over ------------------------------ *
 * A pointer-free description of MAT::Tree (src/mutation_annotated_tree.hpp:80-152):
 * node ids 0..n_nodes-1 in any order, parent[i] = id of the parent or -1 for
 * the single root; the children of a node are ordered by ascending id (the
 * order Tree::create_node pushes them, src/mutation_annotated_tree.cpp:865-878).
 * Node i owns mutations mut_*[mut_off[i] .. mut_off[i+1]), sorted by position
 * (the loader guarantees it, src/mutation_annotated_tree.cpp:591-594), ref_nuc
 * one-hot (src/mutation_annotated_tree.cpp:572) and the same at every mutation
 * of a position;
 * mut_pos < 0 = masked mutation (src/mutation_annotated_tree.hpp:68-70).
 * mut_par (Mutation::par_nuc) may be NULL: the scorer never reads it
 * (src/usher_mapper.cpp:168-506 only copies it), the flattener recomputes the
 * true parent allele. */
typedef struct {
    uint32_t n_nodes;
    const int32_t *parent;     /* [n_nodes]                */
    const uint32_t *mut_off;   /* [n_nodes + 1]            */
    const int32_t *mut_pos;    /* [mut_off[n_nodes]]       */
    const uint8_t *mut_ref;    /* ref_nuc masks            */
    const uint8_t *mut_par;    /* par_nuc masks or NULL    */
    const uint8_t *mut_mut;    /* mut_nuc masks            */
} wepp_tree_desc;

typedef struct wepp_mat wepp_mat_t;   /* flattened MAT resident in one GPU's HBM */

typedef struct {
    uint64_t n_nodes;          /* N                                             */
    uint64_t n_mutations;      /* M: non-masked mutation words                  */
    uint64_t n_masked;         /* masked mutations (kept as node flags only)    */
    uint64_t n_events;         /* E: enter + exit events of the sweep stream    */
    uint64_t n_blocks;         /* sweep blocks (<=64 nodes, <=128 events each)  */
    uint64_t n_leaves;
    uint32_t max_depth;        /* root = 0                                      */
    uint32_t max_position;     /* largest mutated position                      */
    uint64_t stream_bytes;     /* bytes one sweep of the whole-tree stream reads */
    uint64_t device_bytes;     /* total HBM held by the handle                  */
    /* sweep streams: crowns {static score <= tau} closed under ancestors, in
     * increasing tau; the last one is the whole tree (tau = INT32_MAX) */
    uint32_t n_streams;
    int32_t  stream_tau[16];
    uint64_t stream_nodes[16];
    uint64_t stream_bytes_of[16];
    /* window crowns (see wepp_mat_last_crowns): how many were built, their nodes in all */
    uint32_t n_window_crowns;
    uint64_t window_crown_nodes;
    /* window streams (plan class WEPP_PLAN_WIN: tiles of reads with many entries inside one genome window): how many
     * of them are the window's CANDIDATE crown -- the nodes n with out_w(n) - in_w(n) <= score of the root for an
     * empty read, the only ones a read confined to the window can be placed on whatever it lists -- rather than the
     * whole tree as the window sees it, and the elements of all window streams */
    uint32_t n_window_streams;
    uint32_t n_window_streams_crown;
    uint64_t window_stream_nodes;
    /* genome windows: WIN_SIZE positions every WIN_STRIDE (flatmat.hpp; 2560 / 1024 in the product build), at most 32
     * of them: positions from 32 * stride on lie in no window -- window_uncovered_positions of the tree's mutated
     * positions -- and reads there take the tree-wide streams (a SARS-CoV-2 or RSV genome has none) */
    uint32_t window_size, window_stride, window_uncovered_positions;
    /* seed signatures (wepp_mat_set_use_seeds): chunks of the whole-tree stream, blocks per chunk, bytes of the
     * (position x chunk) nibble table; 0 when none was built (genomes beyond 2^18 positions, tables beyond 1 GB) */
    uint32_t seed_chunks, seed_chunk_blocks;
    uint64_t seed_sig_bytes;
} wepp_mat_stats;

/* Per-read result flags (out parameter `flags`). */
#define WEPP_FLAG_HAS_UNIQUE 1u  /* best_node_has_unique, src/usher_common.cpp:374,401 */

/* Build the flat MAT from `tree` and upload it to HIP device `device`.
 * Replaces: MAT::Tree::breadth_first_expansion() per sample
 * (src/usher_common.cpp:339), Tree::get_num_leaves() per tie
 * (src/usher_mapper.cpp:465) and the ancestor walk of every mapper2_body call
 * (src/usher_mapper.cpp:276-287) by a one-time precomputation. */
int wepp_mat_create(const wepp_tree_desc *tree, int device, wepp_mat_t **out);
int wepp_mat_destroy(wepp_mat_t *mat);
int wepp_mat_get_stats(const wepp_mat_t *mat, wepp_mat_stats *out);
/* bfs_ids[k] = caller node id of bfs[k] (breadth_first_expansion order,
 * src/mutation_annotated_tree.cpp:1115-1141); buffer of n_nodes entries. */
int wepp_mat_bfs_order(const wepp_mat_t *mat, uint32_t *bfs_ids);

/* Place a batch of samples/reads: for read r with entries
 * read_word[read_off[r] .. read_off[r+1]) (sorted by position, positions
 * unique -- the precondition of the merge at src/usher_mapper.cpp:205-243)
 * compute what the two passes at src/usher_common.cpp:386-446 leave in
 *     best_j               -> best_bfs_j[r]   (index into the BFS order)
 *     best_set_difference  -> score[r]
 *     num_best             -> num_best[r]
 *     best_node_has_unique -> flags[r] & WEPP_FLAG_HAS_UNIQUE
 * Host buffers in, host buffers out (H2D / D2H inside); synchronous: the
 * results are in the caller's buffers on return.  Batches of 65 536 reads and
 * more run as a pipeline of 2-4 sub-batches (contiguous ranges of the reads):
 * host worker threads the handle starts at the first such call and keeps
 * (wepp_amd/csrc/host_pool.hpp) check and stage the next sub-batch while the
 * previous one's words go up, the one before runs its kernels and the results
 * of the one before that come down and are moved out.  Buffers the caller has
 * pinned (hipHostMalloc / hipHostRegister) are the source / target of the DMA
 * as they stand: no staging pass.  Results never depend on the split.  Any
 * output pointer may be NULL.  per_node_scores, when non-NULL, receives n_reads * n_nodes
 * int32 values: the -p mode's node_set_difference[k] in BFS order
 * (src/usher_common.cpp:403-409, +1 for ineligible nodes src/usher_mapper.cpp:500-505). */
int wepp_place_batch(wepp_mat_t *mat, const uint32_t *read_off, const uint32_t *read_word,
                     uint32_t n_reads, uint32_t *best_bfs_j, int32_t *score, uint32_t *num_best,
                     uint32_t *flags, int32_t *per_node_scores);

/* Imputed mutations of the chosen placement: what pass 2 leaves in
 * node_imputed_mutations[best_j] (src/usher_mapper.cpp:323-378) and
 * usher_common prints as column 4 of placement_stats.tsv
 * (src/usher_common.cpp:764-781).  Every ambiguous (more than one bit set),
 * non-missing entry of a read yields exactly one imputed mutation, in entry
 * order; imp_off[r] .. imp_off[r+1] index imp_pos / imp_nuc (nucleotide masks,
 * one bit set).  best_bfs_j is the placement returned by wepp_place_batch.
 * capacity = size of imp_pos / imp_nuc; WEPP_ELIMIT if too small (the needed
 * size is the number of ambiguous non-missing read words). */
int wepp_imputed_mutations(wepp_mat_t *mat, const uint32_t *read_off, const uint32_t *read_word,
                           uint32_t n_reads, const uint32_t *best_bfs_j, uint32_t *imp_off,
                           int32_t *imp_pos, uint8_t *imp_nuc, uint64_t capacity);

/* best_j_vec: the BFS indices of ALL optimal nodes of every read -- what pass 1 collects for pass 2
 * (src/usher_common.cpp:376-381, filled at src/usher_mapper.cpp:475-476,497; pass 2 loops over it at
 * src/usher_common.cpp:413-446).  `score` / `num_best` are the outputs of wepp_place_batch for the same reads on
 * this handle; best_off[n_reads + 1] receives the CSR over the reads (best_off[r + 1] - best_off[r] = num_best[r]),
 * best_nodes[best_off[r] .. best_off[r + 1]) the optimal nodes of read r in ascending BFS index (the reference's
 * vector is unordered).  capacity = size of best_nodes; WEPP_ELIMIT (best_off filled: best_off[n_reads] is the
 * needed size) when it is too small; WEPP_EINVAL when score / num_best are not this read's placement.
 * Cost: every node of a read's own stream (the crown its bound admits, wepp_mat_stats::stream_nodes) is evaluated
 * once -- a second pass for batches of samples, not for every read of a sequencing run. */
int wepp_best_nodes(wepp_mat_t *mat, const uint32_t *read_off, const uint32_t *read_word, uint32_t n_reads,
                    const int32_t *score, const uint32_t *num_best, uint64_t *best_off, uint32_t *best_nodes,
                    uint64_t capacity);

/* ---- clade assignment of placed samples ------------------------------------------------ *
 * Replaces the loop of src/usher_common.cpp:597-616 (one Tree::get_clade_assignment, src/mutation_annotated_tree.cpp:
 * 923-931, per annotation column and optimal node of a sample, then a sort of the names) for a whole batch.
 * Names never cross this boundary.  For every annotation column c the caller numbers the DISTINCT names of the column,
 * "UNDEFINED" among them, 1, 2, 3 .. BY THEIR RANK UNDER std::string::operator< (byte-wise, a prefix before the longer
 * name): ascending id is then the order in which std::sort leaves Missing_Sample::clade_assignments[c] (:614), and the
 * histograms below come out in the order the -D writer prints them (:937-954).  Any other numbering still counts
 * correctly but lists the clades in another order than the reference.
 *   clade_id[c * n_nodes + caller node id]   0 for a node without annotation in column c, its name's id otherwise
 *   undefined_id[c]                          the id of "UNDEFINED" in column c (what a node without annotated ancestor gets)
 * The call builds and uploads, per column and node, the nearest annotated ancestor including the node and the nearest
 * one excluding it (one top-down pass; once per call, not per sample).  n_columns > 8: WEPP_ELIMIT.  n_columns == 0
 * clears the tables.  Calling again replaces them. */
int wepp_mat_set_clades(wepp_mat_t *mat, uint32_t n_columns, const uint32_t *clade_id, const uint32_t *undefined_id);
/* best_bfs_j = what wepp_place_batch returned for these reads, best_off / best_nodes = what wepp_best_nodes returned.
 * For pair (r, k) with node n = bfs[best_nodes[best_off[r] + k]]: include_self = !n->is_leaf() && !has_unique(r, n)
 * (:607; has_unique as mapper2_body computes it, src/usher_mapper.cpp:184-262), and the pair's clade in column c is the
 * nearest annotated ancestor of n including / excluding n accordingly.
 *   best_clade[c * n_reads + r]   the clade of the pair whose node is best_bfs_j[r]: best_clade_assignment[c] (:610-612)
 *   hist_off[n_columns * n_reads + 1]   CSR over (column, read), segment c * n_reads + r
 *   hist_clade / hist_count       the distinct clades of the read's pairs in ascending id with their counts; the counts
 *                                 of a segment sum to num_best[r]
 * capacity = size of hist_clade / hist_count; WEPP_ELIMIT (best_clade complete, hist_off filled: hist_off[n_columns *
 * n_reads] is the needed size) when it is too small.  WEPP_EINVAL: no clades set on the handle, a best_nodes entry that
 * is no BFS index, best_bfs_j[r] not among read r's nodes.  WEPP_ELIMIT besides: n_columns * (pairs of all reads) or
 * n_columns * (n_reads + 1) >= 2^32; split the batch.  Any output pointer may be NULL (without hist_clade and hist_count
 * the capacity is not looked at; without all three nothing is counted).  Integer work: bit-identical run to run. */
int wepp_clade_assign(wepp_mat_t *mat, const uint32_t *read_off, const uint32_t *read_word, uint32_t n_reads,
                      const uint32_t *best_bfs_j, const uint64_t *best_off, const uint32_t *best_nodes,
                      uint32_t *best_clade, uint64_t *hist_off, uint32_t *hist_clade, uint32_t *hist_count,
                      uint64_t capacity);
/* device time of the calling thread's last wepp_clade_assign by phase (HIP events, ms): the pair kernel; the sorts of
 * the segments, run heads and their scan; run starts, counts and the copies out */
int wepp_clade_last_timing(double *pairs_ms, double *count_ms, double *finish_ms);

/* ---- excess mutations of (sample, node) pairs --------------------------------------- *
 * node_excess_mutations[j] as mapper2_body appends it with compute_vecs for sample
 * pair_read[i] at the node with BFS index pair_bfs_j[i]: first the node's own mutations the
 * sample shares (src/usher_mapper.cpp:223-228, :253-258), then the sample's own alleles the
 * node's genotype does not offer (:357-388, sample order), then back-mutations to the
 * reference (:394-446, position order).  usher prints the first `score` entries for the
 * optimal nodes in the last column of parsimony-scores.tsv (src/usher_common.cpp:555-574).
 * exc_off[n_pairs + 1] is the CSR over the pairs; entry q is
 * MAT::Mutation{position exc_pos[q], ref_nuc exc_ref[q], par_nuc exc_par[q], mut_nuc exc_mut[q]};
 * par_nuc of a node's own mutation is the true parent allele (what Mutation::par_nuc holds
 * in a consistent MAT).  WEPP_ELIMIT (exc_off filled with the needed sizes) when capacity is
 * too small.  Not listed: masked root mutations that carry non-zero nucleotides (the .pb
 * loader zeroes them, src/mutation_annotated_tree.cpp:566-571). */
int wepp_excess_mutations(wepp_mat_t *mat, const uint32_t *read_off, const uint32_t *read_word, uint32_t n_reads,
                          uint32_t n_pairs, const uint32_t *pair_read, const uint32_t *pair_bfs_j,
                          uint64_t *exc_off, int32_t *exc_pos, uint8_t *exc_ref, uint8_t *exc_par, uint8_t *exc_mut,
                          uint64_t capacity);

/* Same computation with every buffer already resident on the handle's device
 * (device pointers); work is enqueued on `hip_stream` (a hipStream_t, NULL =
 * the default stream).  n_read_words = read_off[n_reads].  Used when the caller
 * keeps reads in HBM.
 * Synchronisation: the call BLOCKS the host until the two routing kernels (~20 us per
 * 1 M reads, plus whatever precedes them on the stream) have finished -- the sweep
 * grids are sized from their counters --, then enqueues the sweeps and returns
 * WITHOUT waiting for them: the results are valid once `hip_stream` has reached the
 * point of return.  Work the caller wants overlapped with the routing (the next
 * batch's H2D) goes on another stream. */
int wepp_place_batch_device(wepp_mat_t *mat, const uint32_t *d_read_off, const uint32_t *d_read_word,
                            uint32_t n_reads, uint64_t n_read_words, uint32_t *d_best_bfs_j,
                            int32_t *d_score, uint32_t *d_num_best, uint32_t *d_flags,
                            void *hip_stream);

/* Tuning knob: reads that share one sweep of the event stream (1..64,
 * default 64).  Affects speed only, never results. */
int wepp_mat_set_tile_reads(wepp_mat_t *mat, uint32_t reads_per_tile);
/* Work skipping on (default) / off: when off every read sweeps the whole-tree
 * stream.  Affects speed only, never results. */
int wepp_mat_set_use_crowns(wepp_mat_t *mat, int enable);
/* Per-read walks on (default) / off: when on, a read that lists at most 16 positions visits only the
 * events of those positions (position index + range queries over the stream) instead of sweeping the
 * whole stream with 63 other reads; when off every read is placed by a sweep.  Affects speed only,
 * never results.  WEPP_ELIMIT when enabling on a tree with a stream of 2^25 nodes or more (the walk's interval
 * stack packs a subtree end into 25 bits; such a tree is placed by sweeps). */
int wepp_mat_set_use_walk(wepp_mat_t *mat, int enable);

/* Seeded placement of whole-genome samples on (default) / off.  A sample that lists more positions than a walk takes
 * and fits no genome window -- what read_vcf makes of a consensus genome, src/mutation_annotated_tree.cpp:2033-2130 --
 * is placed by a workgroup of its own: for every chunk (about a thousand nodes) of the whole-tree stream it counts how
 * many of the sample's reference-excluding alleles the chunk's signature -- the alleles carried by the chunk's nodes
 * and the ancestors of its first node -- could serve; a node of the chunk scores at least (such entries) - (count),
 * so only the chunks whose bound reaches the best score found so far are evaluated, node by node, exactly
 * (wepp_amd/csrc/seed_kernels.hip).  Off: such samples share tile sweeps of the whole-tree stream.  Affects speed
 * only, never results. */
int wepp_mat_set_use_seeds(wepp_mat_t *mat, int enable);
/* Diagnostic: samples seeded by the handle since wepp_mat_timing_reset(), the chunks they evaluated, the chunks they
 * could have evaluated (samples x wepp_mat_stats::seed_chunks), the most chunks one sample evaluated, and the samples
 * by chunks evaluated (histogram8: <= 1, <= 4, <= 16, <= 64, <= 256, <= 1024, <= 4096, more).  Any pointer may be
 * NULL.  Synchronises the device. */
int wepp_mat_last_seeds(wepp_mat_t *mat, uint64_t *samples, uint64_t *chunks_evaluated, uint64_t *chunks_total,
                        uint64_t *most_per_sample, uint64_t *histogram8);

/* Tuning knob: sub-batches wepp_place_batch cuts a batch of 65 536 reads or more into (1..8; 0 = default: one per
 * 2 097 152 reads, rounded down, at most 8 -- and at least 2 from 524 288 reads when the handle has two or more host
 * workers; 1 below that).  Sub-batch k runs on the handle's lane k % 2; with two or more host workers a call of several
 * sub-batches launches them from two host threads, one per lane.  Smaller batches and calls that ask for per-node
 * scores are never cut.  Affects speed only, never results. */
int wepp_mat_set_pipeline(wepp_mat_t *mat, uint32_t sub_batches);

/* Timing of the dominant kernel (k_sweep), measured with HIP events recorded on
 * the launch stream around the sweep (+ the 10-80 us finalize) launches of every
 * placement call -- they run concurrently on internal side streams forked from
 * and joined into the launch stream -- since the
 * handle was created or wepp_mat_timing_reset() was called (the most recent 64
 * calls are kept).  Blocks until those launches have finished.
 * mean_sweep_ms = mean duration of the sweep / walk launches of one call; passes =
 * event-stream sweeps of a call (one per tile) plus the 64-read waves of its walks, averaged like the bytes;
 * algorithmic_bytes = bytes the sweeps read (sum over tiles of their stream's size) plus what the walks' lanes
 * asked memory for, counted by the kernel (a 32-byte index entry per node event, the sparse-table bytes and
 * range-query aggregates actually requested, list heads, read words, the start states of the jobs, results),
 * averaged over the calls since the reset. */
int wepp_mat_timing_reset(wepp_mat_t *mat);
int wepp_mat_last_timing(wepp_mat_t *mat, float *mean_sweep_ms, uint32_t *n_calls, uint64_t *passes,
                         uint64_t *algorithmic_bytes);

/* Diagnostic: tiers[r] = index of the sweep stream (wepp_mat_stats::stream_tau) read r of
 * the handle's most recent placement call was routed to; n_reads must be that call's.
 * Synchronises the device.  Lets a test reach every stream with the oracle. */
int wepp_mat_last_tiers(wepp_mat_t *mat, uint8_t *tiers, uint32_t n_reads);

/* Diagnostic: the full plan of every read of the handle's most recent placement call: plan_class[r] = how it was
 * placed (WEPP_PLAN_*), plan_stream[r] = on which stream (index into wepp_mat_stats::stream_tau; for
 * WEPP_PLAN_WIN the index of the genome window).  n_reads must be that call's.  Synchronises the device.  Lets a
 * test reach every (class, stream) pair with the oracle. */
#define WEPP_PLAN_WALK8   0   /* per-read walk, up to 8 listed positions                  */
#define WEPP_PLAN_WALK16  1   /* per-read walk, up to 16                                   */
#define WEPP_PLAN_SWEEP   2   /* sweep of the stream with up to 63 other reads             */
#define WEPP_PLAN_WALKC8  3   /* walk cut into jobs (many events), up to 8 positions       */
#define WEPP_PLAN_WALKC16 4   /* walk cut into jobs, up to 16 positions                    */
#define WEPP_PLAN_WIN     5   /* tile sweep of a genome window's stream (reads with more than 32 entries inside one window) */
#define WEPP_PLAN_SEED    6   /* whole-genome sample: chunk signatures, then exact evaluation of the chunks left (plan_stream 0) */
int wepp_mat_last_plans(wepp_mat_t *mat, uint8_t *plan_class, uint8_t *plan_stream, uint32_t n_reads);
/* plan_stream == WEPP_WINDOW_CROWN_SLOT with a class other than WEPP_PLAN_WIN: the read walked (or, class
 * WEPP_PLAN_SWEEP, swept alone) a WINDOW CROWN -- of the nodes a read confined to its genome window can be placed on at
 * all (at least as many of the path's mutations inside the window as outside), those whose score can be as low as the
 * read's root score (positions outside the window cost every such read the same): far fewer than the tree-wide crown
 * of root score + entries.  wepp_mat_last_crowns tells which for the reads that walked: window[r] = index of the genome
 * window, crown[r] = index of the crown among the window's (increasing bound; the last one admits any root score);
 * 255 / 255 for a read placed otherwise.  (For class WEPP_PLAN_WIN plan_stream is the window's index, which may be 15.) */
#define WEPP_WINDOW_CROWN_SLOT 15
int wepp_mat_last_crowns(wepp_mat_t *mat, uint8_t *window, uint8_t *crown, uint32_t n_reads);

/* Diagnostic: reads of the handle's most recent placement call that walked their own events (k_walk;
 * the others were placed by sweeps of their stream), and the loop iterations (one per event, interval end or
 * range query) all walks of the handle ran since wepp_mat_timing_reset().  Synchronises the device. */
int wepp_mat_last_walk(wepp_mat_t *mat, uint64_t *reads_walked, uint64_t *walk_iterations);

const char *wepp_last_error(void);

/* ---- synthetic workload generators (host only; no GPU needed) ---------- *
 * The reference bundles no MAT or reads; every config is
 * generated deterministically from seeds with a splitmix64 PRNG. */
typedef struct wepp_gen_tree wepp_gen_tree_t;
typedef struct wepp_gen_reads wepp_gen_reads_t;

typedef struct {
    uint64_t seed;
    uint32_t n_nodes;
    uint32_t genome_len;        /* positions 1..genome_len                      */
    double   p_recent_parent;   /* prob. parent is one of the last 8 nodes      */
    double   zipf_s;            /* site-weight exponent (homoplasy skew)        */
    double   p_back_mutation;   /* prob. a mutation at a non-ref site reverts   */
    double   p_ambiguous;       /* prob. a node mutation gets a 2-bit mut_nuc   */
    double   p_masked_node;     /* prob. a non-root node gets a masked mutation */
    uint32_t root_mutations;    /* mutations placed on the root                 */
    /* tree shape (0 = the default shape: uniform attachment, median root path ~20 mutations at 16 M nodes) */
    uint32_t depth_choices;     /* parent = the DEEPEST of this many uniformly drawn earlier nodes: 2 -> paths of ~2x
                                 * the mutations, 16 -> ~5x (real SARS-CoV-2 paths carry 60-100+)              */
    double   p_hub;             /* prob. the parent is one of the tree's hubs instead: polytomies ...           */
    uint32_t n_hubs;            /* ... the first n_hubs nodes (0: n_nodes / 4096 + 1), each ~p_hub * n / n_hubs children */
} wepp_gen_tree_params;

/* shape of a generated tree: mutations on the root path of its leaves, depth, largest polytomy */
typedef struct {
    uint32_t n_nodes, n_leaves, max_depth, max_children;
    uint32_t path_mutations_median, path_mutations_p95, path_mutations_max;
    double   path_mutations_mean, mutations_per_node;
} wepp_gen_tree_shape;

typedef struct {
    uint64_t seed;
    uint32_t n_reads;
    uint32_t read_len;          /* 150 (ARTIC) or ~1200 (midnight)              */
    uint32_t amplicon_len;      /* 400 (ARTIC-like) or 1200 (midnight-like)     */
    uint32_t amplicon_step;     /* tiling step between amplicon starts          */
    double   p_substitution;    /* per-base sequencing error                    */
    double   p_n;               /* per-base N                                   */
    double   p_iupac;           /* prob. an error is an ambiguity code instead  */
} wepp_gen_reads_params;

int wepp_gen_tree_create(const wepp_gen_tree_params *p, wepp_gen_tree_t **out);
int wepp_gen_tree_desc(const wepp_gen_tree_t *t, wepp_tree_desc *out);  /* borrowed pointers */
int wepp_gen_tree_get_shape(const wepp_gen_tree_t *t, wepp_gen_tree_shape *out);
int wepp_gen_tree_destroy(wepp_gen_tree_t *t);

int wepp_gen_reads_create(const wepp_gen_tree_t *t, const wepp_gen_reads_params *p, wepp_gen_reads_t **out);
/* borrowed pointers: read_off[n_reads+1], read_word[read_off[n_reads]] */
int wepp_gen_reads_get(const wepp_gen_reads_t *r, uint32_t *n_reads, const uint32_t **read_off,
                       const uint32_t **read_word);
/* borrowed pointers: the 1-based inclusive genome window [start, end] every read covers
 * (raw_read::start / end for wepp_epp_map) */
int wepp_gen_reads_windows(const wepp_gen_reads_t *r, const int32_t **start, const int32_t **end);
int wepp_gen_reads_destroy(wepp_gen_reads_t *r);

/* ---- per-site Fitch-Sankoff: building a MAT from a tree and a VCF ---------- *
 * Replaces mapper_body::operator() (src/usher_mapper.cpp:7-162), which read_vcf
 * runs once per VCF row when create_new_mat is set
 * (src/mutation_annotated_tree.cpp:1907-2031).  Row s has reference base
 * site_ref[s] (one-hot mask) and names the tree samples
 * var_node[var_off[s] .. var_off[s+1]) (caller node ids) whose allele masks
 * var_nuc[..] differ from the reference or are ambiguous; every other leaf
 * carries the reference base.  The mutation lists of `tree` are ignored.
 * Output: the mutations mapper_body would add (:145-156), as (row, node id,
 * par_nuc mask, mut_nuc mask), rows in order and BFS order inside a row.
 * *n_out receives their number; WEPP_ELIMIT (with *n_out set) when capacity is
 * too small: nothing is then written to the output arrays, and never more than
 * `capacity` entries are.
 * The var_node of a row may come in any order; a node named more than once in a
 * row keeps its LAST entry (:48-63); node ids need not follow any traversal
 * order (the root need not be 0, a parent may have a larger id than its child).
 * Limits: < 2^28 nodes.  A tree of any depth is accepted as long as every
 * observed allele set is non-empty and no node has more than 32767 children
 * (the level-synchronous kernels); rows with an empty allele set, or a larger
 * polytomy, need the kernels with an LDS stack: tree depth <= 140, else
 * WEPP_ELIMIT from the run (the plan stays usable). */
int wepp_fitch_sites(const wepp_tree_desc *tree, int device, uint32_t n_sites, const uint8_t *site_ref,
                     const uint32_t *var_off, const uint32_t *var_node, const uint8_t *var_nuc,
                     uint64_t capacity, uint64_t *n_out, uint32_t *out_site, uint32_t *out_node,
                     uint8_t *out_par, uint8_t *out_mut);

/* The same with the tree-dependent work done once: read_vcf runs mapper_body row after row on ONE tree
 * (src/mutation_annotated_tree.cpp:1962-2031); a plan keeps the flattened topology, the level tables and the
 * decision-table memory on the device, so that repeated calls (batches of VCF rows) only pay for their rows.
 * wepp_fitch_sites == create + run + destroy.  A plan is bound to one device and is not re-entrant. */
typedef struct wepp_fitch_plan wepp_fitch_plan_t;
int wepp_fitch_plan_create(const wepp_tree_desc *tree, int device, wepp_fitch_plan_t **out);
int wepp_fitch_plan_run(wepp_fitch_plan_t *plan, uint32_t n_sites, const uint8_t *site_ref, const uint32_t *var_off,
                        const uint32_t *var_node, const uint8_t *var_nuc, uint64_t capacity, uint64_t *n_out,
                        uint32_t *out_site, uint32_t *out_node, uint8_t *out_par, uint8_t *out_mut);
int wepp_fitch_plan_destroy(wepp_fitch_plan_t *plan);
/* wall time of the calling thread's last wepp_fitch_plan_run by phase (ms): host preparation of the rows, uploads,
 * kernels, sort + decode + copy-out of the mutations */
int wepp_fitch_last_timing(double *prep_ms, double *upload_ms, double *kernels_ms, double *output_ms);
/* debug query: what the calling thread's last wepp_fitch_plan_run that reached the kernels did.  form = one of
 * WEPP_FITCH_FORM_* (-1 before any run), chunks = DFS chunks of the stack forms (0 for the level form), groups = how
 * many groups of batches the rows were cut into, duplicates_dropped = 1 when some row named a node more than once */
#define WEPP_FITCH_FORM_LEVELS 0
#define WEPP_FITCH_FORM_SETS 1
#define WEPP_FITCH_FORM_SCORES 2
int wepp_fitch_last_run_info(int *form, uint32_t *chunks, uint32_t *groups, int *duplicates_dropped);

/* ---- WEPP's own read placement: EPP sets and haplotype scores -------------- *
 * Replaces wepp_filter::cartesian_map (src/WEPP/initial_filter.cpp:140-239) with
 * single_read_tree (:41-136), the range trees it walks (src/WEPP/arena.cpp:68-169)
 * and the per-read distance haplotype::mutation_distance (src/WEPP/haplotype.hpp:
 * 123-173).  `mat` is created from the CONDENSED tree (create_condensed_tree,
 * src/WEPP/util.cpp:79-133): one node per haplotype; haplotypes are addressed by
 * their arena index = pre-order index (arena::from_mat, arena.cpp:3-55), which
 * wepp_mat_dfs_order maps to caller node ids.
 * A read is a raw_read (src/WEPP/read.hpp:8-14): genome window [start, end]
 * (1-based, inclusive), multiplicity `degree`, and one packed word
 * (wepp_pack_read_word, mut_nuc 15 = N) per position where it differs from the
 * reference, sorted by position.
 * Outputs (all host buffers):
 *   max_parsimony[R]   wepp_filter::max_parismony: smallest windowed distance (:203)
 *   multiplicity[R]    parsimony_multiplicity: number of haplotypes attaining it (:204)
 *   epp_off/epp_nodes  epp_positions_cache: ascending arena indices of those
 *                      haplotypes for every read with multiplicity <= max_cached_epp
 *                      (MAX_CACHED_EPP_SIZE = 2048, config.hpp:9), CSR over the reads;
 *                      both may be NULL
 *   hap_score[N]       haplotype::score = sum over reads of
 *                      degree / ((1 + parsimony) * multiplicity) (initial_filter.hpp:54-57);
 *                      accumulated in 64-bit fixed point: run-to-run identical, exact zeros,
 *                      absolute error <= (reads mapped to the haplotype) * 2^-(42 - log2(sum of degrees))
 *   hap_read_counts[N*50]  haplotype::mapped_read_counts (bin = min(start / (genome_size / 50), 49)); may be NULL
 *   hap_divergence[N]  haplotype::dist_divergence (:224-233); may be NULL
 * The final sort of the haplotypes by score (:236) is left to the caller.
 * Preconditions (WEPP_EINVAL otherwise): listed alleles differ from the reference base,
 * positions sorted and unique, 1 <= start <= end, genome_size >= 50. */
#define WEPP_NUM_RANGE_BINS 50
#define WEPP_MAX_CACHED_EPP_SIZE 2048
typedef struct {
    uint32_t n_reads;
    const uint32_t *read_off;   /* [n_reads + 1] */
    const uint32_t *read_word;  /* [read_off[n_reads]] */
    const int32_t *start;       /* [n_reads] raw_read::start */
    const int32_t *end;         /* [n_reads] raw_read::end   */
    const int32_t *degree;      /* [n_reads] raw_read::degree */
} wepp_epp_reads;
typedef struct {
    int32_t *max_parsimony;
    uint32_t *multiplicity;
    uint64_t *epp_off;          /* [n_reads + 1] or NULL */
    uint32_t *epp_nodes;        /* [epp_capacity] or NULL */
    uint64_t epp_capacity;
    double *hap_score;
    int32_t *hap_read_counts;   /* node-major [N][50] or NULL */
    double *hap_divergence;     /* or NULL */
} wepp_epp_out;
int wepp_epp_map(wepp_mat_t *mat, const wepp_epp_reads *reads, uint32_t genome_size, uint32_t max_cached_epp,
                 wepp_epp_out *out);
/* The size of the EPP lists is only known once the map has run (the sum of the multiplicities <= max_cached_epp).
 * When epp_nodes is too small (epp_capacity < epp_off[n_reads]; epp_capacity = 0 with epp_nodes = NULL asks for
 * exactly that) wepp_epp_map still delivers EVERY other output, keeps the lists on the handle and returns
 * WEPP_ELIMIT; the caller sizes its buffer from epp_off[n_reads] and collects them here -- the map never runs twice.
 * The pending lists belong to the handle's most recent wepp_epp_map and are dropped by the fetch. */
int wepp_epp_fetch_lists(wepp_mat_t *mat, uint32_t *epp_nodes, uint64_t capacity);
/* caller node id of the haplotype with arena (pre-order) index k, for k = 0 .. n_nodes-1 */
int wepp_mat_dfs_order(const wepp_mat_t *mat, uint32_t *ids);
/* device time of the calling thread's last wepp_epp_map, by phase (HIP events), and its work:
 * events_swept = sum over tiles of the window-stream events one tile walks per pass */
int wepp_epp_last_timing(double *select_ms, double *sweep1_ms, double *sweep2_ms, double *finish_ms,
                         uint64_t *events_swept, uint64_t *stream_events, uint32_t *groups, uint32_t *jobs);

/* ---- reads against a selection of haplotypes ------------------------------- *
 * Replaces the loop of arena::dump_read2haplotype_mapping (src/WEPP/arena.cpp:610-667;
 * the same loop in arena::resolve_unaccounted_mutations, :833-866): every read against
 * every SELECTED haplotype through haplotype::mutation_distance (src/WEPP/haplotype.hpp:
 * 123-177).  How the selection was made (peak loop, Freyja, a list the user brings) is the
 * caller's business.  `mat` is the handle of the condensed tree, `reads` a batch as for
 * wepp_epp_map, sel[0 .. n_sel) distinct arena (pre-order) indices in the caller's order
 * (the reference's `abundance` order).  d(r, k) = the distance of read r to haplotype
 * sel[k], whose stack_muts are as arena::from_mat builds them (arena.cpp:17-48): the
 * deepest mutation of the root path wins at a position and is kept when mut_nuc != ref_nuc.
 * Outputs (all host buffers):
 *   min_dist[R]      min over k of d(r, k)                        (arena.cpp:614-625)
 *   n_epp[R]         number of k attaining it
 *   asg_off/asg_sel  the reference's `epps` per read: the indices INTO sel attaining the
 *                    minimum, ascending, as a CSR over the reads (asg_off[R + 1]); both or
 *                    neither -- asg_off alone with asg_capacity = 0 asks for the sizes only
 *   sel_reads[K]     reads whose set holds k
 *   sel_degree[K]    sum of their degree                          (the count of :859-865)
 *   sel_covered[K]   sites j, 1 <= j <= genome_size, inside [start, end] of at least one
 *                    read assigned to k at which that read lists no N (:637-665); the
 *                    coverage file holds sel_covered / genome_size (:681-688)
 *   cover_bits       the coverage bitmaps themselves, K rows of ceil(genome_size / 32)
 *                    words, bit (j - 1) & 31 of word (j - 1) / 32 for site j; may be NULL.
 *                    Shards of a read set are combined by OR (sel_reads / sel_degree by +).
 * Everything is integer and independent of the order of execution: bit-identical run to run.
 * Preconditions on the reads: those of wepp_epp_map, same codes and messages; genome_size
 * >= 1 (the 50-bin rule belongs to the map).  WEPP_EINVAL: n_sel == 0, an index >= n_nodes,
 * a repeated index.  WEPP_ELIMIT: the device table of the selection (3 bytes per tree
 * position and haplotype, columns padded to 256) would exceed 1 GiB -- assign to the
 * selection in parts --; a selected haplotype with more than 65535 non-reference positions
 * (16-bit prefix counts); asg_capacity < asg_off[n_reads] -- then EVERY other output is
 * delivered, asg_off is filled, and the caller calls again with a buffer of asg_off[n_reads]
 * entries: nothing is kept pending on the handle, a second call is cheap here, unlike the map.
 * n_reads == 0: the per-haplotype outputs are zero, asg_off[0] = 0.  Serial per handle, like
 * wepp_epp_map, whose device block cache it shares. */
typedef struct {
    int32_t *min_dist; uint32_t *n_epp;          /* [n_reads] */
    uint64_t *asg_off; uint32_t *asg_sel; uint64_t asg_capacity;   /* both or neither */
    uint32_t *sel_reads; int64_t *sel_degree; uint32_t *sel_covered;   /* [n_sel] */
    uint32_t *cover_bits;                         /* [n_sel * ceil(genome_size/32)] or NULL */
} wepp_assign_out;
int wepp_epp_assign(wepp_mat_t *mat, const wepp_epp_reads *reads, uint32_t genome_size,
                    uint32_t n_sel, const uint32_t *sel, wepp_assign_out *out);
/* device time of the calling thread's last wepp_epp_assign by phase (HIP events, ms): the selection's
 * genotype table, reads x selection (k_assign), lists + coverage counts */
int wepp_epp_assign_last_timing(double *tables_ms, double *assign_ms, double *finish_ms);

/* ---- residual mutations against a selection of haplotypes ------------------ *
 * Replaces arena::resolve_unaccounted_mutations (src/WEPP/arena.cpp:739-892) up to its two files: which
 * reads carry each residual mutation (an allele seen in the reads that the selected haplotypes do not
 * explain) and which selected haplotypes it most plausibly belongs to.  `mat`, `reads`, `genome_size` and
 * `sel` are those of wepp_epp_assign; res_word[0 .. n_res) are the residual mutations IN THE CALLER'S ORDER,
 * each wepp_pack_read_word(position, ref_nuc, mut_nuc, 0): ref_nuc the one-hot mask of the reference base at
 * the position, mut_nuc the residual allele's mask, 1 .. 14.
 * For every read r start from a copy r' of its entries and visit the m with start <= pos(m) <= end in
 * increasing m (the reference's copy_if order; it matters when two residual mutations share a position):
 *   r' has an entry at pos(m) that is not N: if its mut_nuc == mut_nuc(m) the entry becomes N and r is
 *     COVERED for m (:765-770); otherwise nothing happens;
 *   r' has an N entry at pos(m) -- also one an earlier m' at the position has just made --: r is MASKED
 *     for m (:773-775);
 *   r' has no entry at pos(m): if mut_nuc(m) == ref_nuc(m) an N entry is inserted in position order and r
 *     is covered (:780-790); otherwise nothing happens.
 * The final r' stands for r under every m it is covered or masked for (:794-807); a read with no relation
 * takes no further part.  With S(m) the covered and masked reads of m and epps(r') the k minimising
 * wepp_epp_assign's d(r', k):
 *   rel_off/rel_read   S(m) as a CSR over the mutations: read indices ascending within a mutation, bit 31
 *                      set = masked, clear = covered; both or neither, rel_off alone with rel_capacity = 0
 *                      asks for the sizes only
 *   n_covered[M], n_masked[M]
 *   hap_reads[M * K]   reads of S(m) whose epps hold k; may be NULL
 *   hap_degree[M * K]  sum of their degree (:859-865); may be NULL
 *   best_degree[M]     max of hap_degree[m][k] over the k with hap_reads[m][k] > 0; 0 when S(m) is empty
 *   best_mask          [M * ceil(K / 32)], bit k & 31 of word k / 32: hap_reads[m][k] > 0 and hap_degree[m][k]
 *                      == best_degree[m] (the reference's map only holds haplotypes that appeared, :859-884:
 *                      a mutation whose reads all have degree 0 lists those, not all K)
 *   n_touched[1]       reads with at least one relation
 * Everything is integer: bit-identical run to run.  Read shards: hap_reads / hap_degree add, best_* must be
 * recomputed from the sums.  The argument checks on reads and selection and the table limits are
 * wepp_epp_assign's.  WEPP_EINVAL besides: a residual position outside 1 .. genome_size, mut_nuc 0 or 15,
 * ref_nuc not one-hot.  WEPP_ELIMIT besides: n_reads >= 2^31; 2^32 or more entries in the touched reads
 * after the insertions; rel_capacity < rel_off[n_res] -- then EVERY other output is delivered and rel_off is
 * filled, as with asg_sel.  n_res == 0, n_reads == 0 or no touched read: WEPP_OK, zeroed outputs, rel_off all
 * 0, no assignment is launched.  Serial per handle. */
typedef struct {
    uint64_t *rel_off;      /* [n_res + 1] */
    uint32_t *rel_read;     /* [rel_capacity] */
    uint64_t rel_capacity;
    uint32_t *n_covered;    /* [n_res] */
    uint32_t *n_masked;     /* [n_res] */
    int64_t  *best_degree;  /* [n_res] */
    uint32_t *best_mask;    /* [n_res * ceil(n_sel / 32)] */
    uint32_t *hap_reads;    /* [n_res * n_sel] or NULL */
    int64_t  *hap_degree;   /* [n_res * n_sel] or NULL */
    uint32_t *n_touched;    /* [1] */
} wepp_resolve_out;
int wepp_epp_resolve(wepp_mat_t *mat, const wepp_epp_reads *reads, uint32_t genome_size,
                     uint32_t n_sel, const uint32_t *sel,
                     uint32_t n_res, const uint32_t *res_word, wepp_resolve_out *out);
/* device time of the calling thread's last wepp_epp_resolve by phase (HIP events, ms): marking the reads and
 * ordering the relations, the selection's genotype table, k_assign on the touched reads, tally + best */
int wepp_epp_resolve_last_timing(double *mark_ms, double *tables_ms, double *assign_ms, double *tally_ms);

/* ---- haplotypes within a mutation radius of pivots ------------------------- *
 * The primitive under arena::closest_neighbors and arena::highest_scoring_neighbors (src/WEPP/arena.cpp:171-249):
 * all haplotypes within mutation distance `radius` of a pivot that are reachable from it through haplotypes
 * within the radius.  piv[0 .. n_piv) are distinct arena indices.  With g_h(p) the allele mask of haplotype h at
 * position p as arena::from_mat builds stack_muts (0 = the reference base, also after a back-mutation),
 * haplotype::mutation_distance(haplotype*) (haplotype.hpp:179) is asymmetric where an allele is N (15); `form`
 * chooses the direction the caller's loop uses:
 *   WEPP_NBR_TO_PIVOT    D(n) = node->mutation_distance(pivot) = sum over p of [g_piv(p) != 15][g_n(p) != g_piv(p)]
 *                        (closest_neighbors)
 *   WEPP_NBR_FROM_PIVOT  D(n) = pivot->mutation_distance(node) = sum over p of [g_n(p) != 15][g_n(p) != g_piv(p)]
 *                        (highest_scoring_neighbors)
 * The REGION of a pivot is its connected component in the forest the tree induces on {n : D(n) <= radius}: what
 * the reference's BFS over parent and children, and its climb followed by the pruned DFS, both enumerate.
 *   nbr_off/nbr_node/nbr_dist  the regions as a CSR over the pivots (nbr_off[n_piv + 1]): arena indices
 *                        ascending within a pivot, with their D.  Nodes with skip[n] != 0 are walked through but
 *                        not listed (include_mapped = false); skip may be NULL.  The pivot itself is listed
 *                        unless it is skipped.  nbr_off alone with nbr_capacity = 0 asks for the sizes only.
 *   top[n_piv]           the highest ancestor of the pivot in its region; may be NULL
 *   n_region[n_piv]      size of the region before `skip`; may be NULL
 * The ranking by score and the num_limit truncation are the caller's, like the final sort of wepp_epp_map.
 * Everything is integer and independent of the order of execution: bit-identical run to run.
 * The pivots are processed in passes of as many as fit a device budget of 2 GiB (8 bytes per tree node and
 * pivot); WEPP_NBR_PASS_COLS in the environment (diagnostic, read once per handle, changes no result) forces the
 * number of pivots per pass.  WEPP_EINVAL: a null argument, n_piv == 0, an index >= n_nodes, a repeated pivot, an
 * unknown form.  WEPP_ELIMIT: a tree of which not even 4 pivots fit the budget; the table limits of
 * wepp_epp_assign for the pivots of a pass; nbr_capacity < nbr_off[n_piv] -- then EVERY other output is delivered,
 * nbr_off is filled, and the caller calls again: nothing stays pending on the handle.  Serial per handle. */
#define WEPP_NBR_TO_PIVOT   0
#define WEPP_NBR_FROM_PIVOT 1
typedef struct {
    uint64_t *nbr_off;      /* [n_piv + 1] */
    uint32_t *nbr_node;     /* [nbr_capacity] */
    int32_t  *nbr_dist;     /* [nbr_capacity] */
    uint64_t nbr_capacity;
    uint32_t *top;          /* [n_piv] or NULL */
    uint32_t *n_region;     /* [n_piv] or NULL */
} wepp_neighbors_out;
int wepp_epp_neighbors(wepp_mat_t *mat, uint32_t n_piv, const uint32_t *piv, uint32_t radius, int form,
                       const uint8_t *skip /* [n_nodes] or NULL */, wepp_neighbors_out *out);
/* the whole distance field, dist[k * n_nodes + n] = D(n) of pivot k: for small trees, tests and
 * print_mutation_distance-style reports.  WEPP_ELIMIT beyond 2^28 cells (n_piv * n_nodes). */
int wepp_epp_distances(wepp_mat_t *mat, uint32_t n_piv, const uint32_t *piv, int form, int32_t *dist);
/* device time of the calling thread's last wepp_epp_neighbors / wepp_epp_distances by phase, summed over the
 * passes (HIP events, ms): the pivots' genotype tables, the distance field (deltas + column scan), the regions
 * (radius test, second scan, tops, counts, lists) */
int wepp_epp_neighbors_last_timing(double *tables_ms, double *field_ms, double *region_ms);

/* ---- the peak-removal loop -------------------------------------------------- *
 * Replaces `while (!step(...))` of wepp_filter::filter (src/WEPP/initial_filter.cpp:467-469): step, singular_step,
 * find_correspondents, remove_read and clear_neighbors (:241-453).  The call runs wepp_epp_map itself (the
 * fixed-point sums behind hap_score, P = max_parsimony, M = multiplicity and the share q[r] every EPP haplotype of
 * read r received stay on the device) and delivers the map's outputs too when map_out is given (lists for reads with
 * multiplicity <= WEPP_MAX_CACHED_EPP_SIZE; a short epp_nodes ends the call with WEPP_ELIMIT before the loop).
 * With d(r, h) the distance of wepp_epp_assign, a haplotype LIVE when it is not mapped and its score is
 * > score_epsilon, and full_score = score * sqrt(dist_divergence) (haplotype.hpp:183-185), one step is:
 *   1. m = the largest full_score over the live haplotypes; the loop ends when there is none or m < score_epsilon.
 *      The tie group = the live haplotypes with m - full_score < score_epsilon, ordered by tie_rank ascending (the
 *      place score_comparator, arena.hpp:16-31, gives them through leaf_count and id), lower arena index first among
 *      equal ranks and when tie_rank is NULL.  (The device gathers the group unordered; the ordering and the walk
 *      of step 2 run on the host, so the whole group crosses to the host and back once per step.)
 *   2. the group is walked in that order while fewer than top_n are accepted and accepted + peaks < max_peaks; a
 *      candidate c is accepted iff old->mutation_distance(c) > peak_radius for every accepted old (the distance of
 *      WEPP_NBR_FROM_PIVOT with pivot old).  The accepted become mapped and join the peaks in this order.
 *   3. every haplotype of the WEPP_NBR_FROM_PIVOT region of radius peak_radius of every accepted peak becomes mapped.
 *   4. every remaining read r with d(r, a) == P[r] for an accepted a leaves the remaining set; it belongs to the FIRST
 *      such a in the order of step 2, and every haplotype h with d(r, h) == P[r] loses exactly q[r].
 *   5. the loop ends when peaks >= max_peaks or no read remains.
 * Outputs: peaks / peak_step / peak_reads / peak_degree / peak_score in selection order (peak_score = the full_score
 * when chosen, peak_reads / peak_degree = the reads removed for the peak and the sum of their degrees); n_steps = the
 * steps that accepted a peak; removed_step[r] / removed_peak[r] = the step and the place in `peaks` of the peak that
 * took read r, -1 / 0xFFFFFFFF for a read that remains; mapped[n]; score_left[n] = the score when the loop ended
 * (fixed point like hap_score: exactly 0 for a haplotype whose reads are all gone; the scores of mapped haplotypes,
 * which the reference leaves dependent on its cache, are those of this closed form).
 * Near ties: the sums are integers, so haplotypes with the same EPP reads tie exactly.  The result is the reference's
 * whenever, at every step, each live full_score is either within a hair of m or clearly (by more than the fixed-point
 * error of hap_score) more than score_epsilon below it; in between the reference's own parallel_sort under a
 * comparator that is no strict weak order decides, and no port can promise its answer.
 * Conventions: those of wepp_epp_map (codes, messages, limits) and of wepp_epp_assign for the peaks' genotype table.
 * n_reads == 0: no peaks, WEPP_OK.  top_n == 0 or max_peaks == 0: WEPP_EINVAL.  Serial per handle. */
typedef struct { uint32_t top_n, max_peaks, peak_radius; double score_epsilon; } wepp_peaks_params;
   /* defaults 10, 300, 2, 1e-9: TOP_N, MAX_PEAKS, MAX_PEAK_PEAK_MUTATION, SCORE_EPSILON of src/WEPP/config.hpp */
typedef struct {
    uint32_t *n_peaks, *n_steps, *n_remaining;      /* [1] each */
    uint32_t *peaks, *peak_step, *peak_reads;       /* [max_peaks], selection order */
    int64_t  *peak_degree;  double *peak_score;     /* [max_peaks] */
    int32_t  *removed_step; uint32_t *removed_peak; /* [n_reads] */
    uint8_t  *mapped;                               /* [n_nodes] */
    double   *score_left;                           /* [n_nodes] or NULL */
} wepp_peaks_out;
int wepp_epp_peaks(wepp_mat_t *mat, const wepp_epp_reads *reads, uint32_t genome_size, const wepp_peaks_params *params,
                   const uint32_t *tie_rank /* [n_nodes] or NULL */, wepp_epp_out *map_out /* or NULL */,
                   wepp_peaks_out *out);
/* wall time of the calling thread's last wepp_epp_peaks by phase (ms; every phase ends with the device idle): the map;
 * leaders, tie groups and the accepted peaks' distance fields; the reads of the accepted peaks; their removal from
 * the scores (the map's sweep over the subset); the regions that become mapped */
int wepp_epp_peaks_last_timing(double *map_ms, double *select_ms, double *hits_ms, double *remove_ms, double *clear_ms);

/* ---- aligned reads to merged reads (sam2PB without the parse) ---------------- *
 * Replaces sam::build behind sam::add_reads (src/WEPP/sam2pb.cpp:262-275, 281-314, 456-470 with operator< / == of
 * sam2pb.hpp:33-47) under the reference's constants USE_READ_CORRECTION, USE_COLUMN_MERGING,
 * !MAP_TO_MAJORITY_INSTEAD_OF_N and SCORE_EPSILON = 1e-9.  No tree handle: the call runs on HIP device `device`.
 * Input: `reference` = the genome_size characters of the reference as dataset::reference delivers them (ASCII, upper
 * case); aligned read r starts at the 0-based site start[r] and holds the columns base[base_off[r] .. base_off[r+1]),
 * one byte 0..5 = "ACGTN_" each (sam2pb.hpp:10).
 *   1. freq[site * 6 + c] = the columns with character c at the site, c != N (the N column stays 0, '_' is counted).
 *   2. total = the six columns' sum; a column with character c becomes N when min_depth > total, else when
 *      min_af - (double)freq[c] / (double)total > 1e-9 (IEEE fp64 as written: total == 0 gives NaN, the comparison is
 *      false and the column stays); then '_' becomes N.  (The table update of :316-328 feeds only dead code: not built.)
 *   3. the reads are ordered by start, then length, then the corrected string in ASCII order (A < C < G < N < T);
 *      reads equal in (start, string) merge into one whose degree is their number.
 * Outputs (host buffers): freq (the RAW table of step 1; may be NULL); order[s] = the input read at place s of the
 * order; n_merged; group_off[g] .. group_off[g + 1] = the places of merged read g (group_off holds n_reads + 1
 * entries, n_merged + 1 are written); and the merged batch in the fields of wepp_epp_reads -- start = start + 1,
 * end = start + length - 1, degree, and one word (wepp_pack_read_word, position 1-based, ref_nuc / mut_nuc the
 * nucleotide masks of the two characters, 15 and is_missing for N) per column whose corrected character differs from
 * the reference character: what load_reads_from_proto (:489-549) makes of the file sam::dump_proto writes.
 * Departures from the reference: among equal reads the one earliest in the input leads the group (order lists the
 * members of a group by ascending input index; the reference's unstable sort leaves both open).  This call takes
 * every read it is given; subsampling (:362-454) is wepp_sam_build_subsampled below, with a defined draw.
 * A read_word buffer that is too small (word_capacity < read_off[n_merged]; 0 with read_word = NULL asks for exactly
 * that) follows wepp_epp_map's protocol: EVERY other output is delivered, the words wait in the calling thread and
 * the call returns WEPP_ELIMIT; wepp_sam_fetch_words collects them (and drops them) without recomputing.
 * WEPP_EINVAL: a null argument, a base byte > 5, a read outside [0, genome_size), an empty read, base_off[0] != 0 or
 * offsets that do not ascend.  WEPP_ELIMIT: genome_size > WEPP_MAX_POSITION (the words' 20-bit positions),
 * n_reads >= 2^31, 2^32 or more words in the merged reads.  n_reads == 0: WEPP_OK, n_merged = 0, freq zeroed.
 * The pile-up reads every read's window once per tile of 2048 sites: the cost grows with genome_size / 2048. */
typedef struct {
    uint32_t n_reads;
    const uint32_t *start;      /* [n_reads] 0-based site of the first column */
    const uint64_t *base_off;   /* [n_reads + 1] */
    const uint8_t *base;        /* [base_off[n_reads]] 0..5 = ACGTN_ */
} wepp_sam_reads;
typedef struct { double min_af; uint32_t min_depth; } wepp_sam_params;   /* dataset::min_af (a float, widened), min_depth */
typedef struct {
    int32_t *freq;              /* [genome_size * 6] or NULL */
    uint32_t *n_merged;         /* [1] */
    uint32_t *order;            /* [n_reads] */
    uint32_t *group_off;        /* [n_reads + 1] */
    uint32_t *read_off;         /* [n_reads + 1]; the five fields of wepp_epp_reads, n_merged reads */
    uint32_t *read_word;        /* [word_capacity] or NULL */
    int32_t *start;             /* [n_reads] */
    int32_t *end;               /* [n_reads] */
    int32_t *degree;            /* [n_reads] */
    uint64_t word_capacity;
} wepp_sam_out;
int wepp_sam_build(int device, const uint8_t *reference, uint32_t genome_size, const wepp_sam_reads *reads,
                   const wepp_sam_params *params, wepp_sam_out *out);
int wepp_sam_fetch_words(uint32_t *read_word, uint64_t capacity);
/* device time of the calling thread's last wepp_sam_build by phase (HIP events, ms): the pile-up with the keep table;
 * the correction (word counts, their scan, the words); the sort; the merge (flags, scans, the merged batch) */
int wepp_sam_last_timing(double *pileup_ms, double *correct_ms, double *sort_ms, double *merge_ms);

/* ---- read subsampling in front of sam::build -------------------------------- *
 * Replaces sam::subsample (src/WEPP/sam2pb.cpp:362-454, SUBSAMPLE_ITERS of config.hpp:6) in front of sam::build: of
 * n = n_reads > m = max_reads aligned reads, T = trials subsets of m reads are drawn, each is piled up into a table of
 * its own, and the subset whose allele frequencies have the smallest KL divergence from the whole sample's is kept;
 * the kept reads are then corrected, sorted and merged as wepp_sam_build does it.
 * The draw.  f(x) is the splitmix64 finaliser on 64-bit unsigned integers:
 *     x += 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;
 *     return x ^ x >> 31;                                           (f(0) = 0xE220A8397B1DCDAF)
 * For trial t, h_t = f(seed ^ f(t)) and key(t, r) = f(h_t ^ r) for the read of input index r.  f is a bijection, so
 * the keys of a trial are distinct; the subset of trial t is the m reads of the smallest keys, that is
 * key(t, r) <= thr_t with thr_t the m-th smallest key.  A trial's subset depends on seed, t, n and m alone.
 * The divergence.  F = the raw table of wepp_sam_build step 1 (N not counted, '_' counted), S_i its six columns' sum
 * at site i, C the number of sites with S_i > 0.  A_t = the same pile-up over the subset of trial t with N counted
 * too (:419-426), A_i and C_t likewise.  p_ij = F_ij / (S_i * C), q_ij = A_ij / (A_i * C_t) and 0 when A_i = 0,
 *     D_t = the sum over the cells with F_ij > 0 of p_ij * (ln p_ij - ln max(q_ij, 1e-10))            (:377-392, :429-439)
 * in IEEE fp64, every operation as written.  The sum is taken in a fixed order without atomics: D_t is a function of
 * the two tables alone, so trials with equal tables get bit-equal divergences; against a sum of the same terms taken
 * exactly it is off by rounding only.  The winner is the trial of the smallest D_t, the lowest t among equals.
 * After the pick the kept reads go through steps 2 and 3 of wepp_sam_build, the keep table of step 2 taken from the
 * FULL table F (the reference leaves collapsed_frequency_table as it was, :394, :281-314).
 * Outputs: `out` as for wepp_sam_build with two differences: freq is the full raw table F, and order[s] for
 * s < n_kept names INPUT reads while group_off and the merged batch range over the kept reads (places 0 .. n_kept).
 * n_kept = m; kept = the ascending input indices of the kept reads; best_trial; divergence[t] = D_t and
 * threshold[t] = thr_t for every trial (either may be NULL).  The word-buffer protocol is wepp_sam_build's
 * (WEPP_ELIMIT, wepp_sam_fetch_words), and wepp_sam_last_timing reports the full pile-up and the stages over the kept
 * reads.
 * n_reads <= max_reads: nothing is drawn, the call is wepp_sam_build: the same outputs, n_kept = n_reads, kept the
 * identity, best_trial = UINT32_MAX, divergence and threshold zeroed.
 * Departures from the reference: the draw is the seeded hash order above, not std::shuffle of an mt19937 seeded from
 * std::random_device (which has no defined result); ties go to the lowest trial, where the reference's winner among
 * equals depends on thread timing.
 * WEPP_EINVAL, besides those of wepp_sam_build: max_reads == 0, trials == 0, a null sub / sub_out / n_kept /
 * best_trial / kept.  WEPP_ELIMIT, besides those: trials > 65 536.
 * On the device the trials' tables (genome_size * 24 bytes each) are worked off in passes of consecutive trials that
 * hold at most 256 MiB of tables (SUB_PASS_BYTES, wepp_amd/csrc/sam_subsample.hpp; at least 8 trials a pass).
 * WEPP_SAM_SUBSAMPLE_PASS_BYTES in the environment (diagnostic, read once per call) lowers the bound; the results do
 * not depend on it. */
typedef struct { uint64_t seed; uint32_t max_reads; uint32_t trials; } wepp_sam_subsample_params;
typedef struct {
    uint32_t *n_kept;       /* [1] */
    uint32_t *kept;         /* [max_reads] ascending input indices of the kept reads */
    uint32_t *best_trial;   /* [1]; UINT32_MAX when nothing was drawn */
    double   *divergence;   /* [trials] or NULL */
    uint64_t *threshold;    /* [trials] or NULL: thr_t */
} wepp_sam_subsample_out;
int wepp_sam_build_subsampled(int device, const uint8_t *reference, uint32_t genome_size, const wepp_sam_reads *reads,
                              const wepp_sam_params *params, const wepp_sam_subsample_params *sub,
                              wepp_sam_out *out, wepp_sam_subsample_out *sub_out);
/* device time of the calling thread's last wepp_sam_build_subsampled by phase (HIP events, ms; zero when nothing was
 * drawn): the thresholds; the tiles' read lists with the trial pile-ups and divergences; the pick with the compaction
 * of the kept reads */
int wepp_sam_subsample_last_timing(double *select_ms, double *trials_ms, double *pick_ms);

/* ---- pairwise distances between genotypes (haplotype uncertainty, truth report) ---- *
 * The primitive behind dump_haplotype_uncertainty (src/WEPP/arena.cpp:494-528) and print_mutation_distance
 * (:251-301): mutation_distance over get_mutations (src/WEPP/util.cpp:188-222, 271-296), taken over all pairs of a
 * group or over A x B.  No tree handle: the calls run on HIP device `device`; the caller lists the genotypes.
 * A genotype is the list of a node's differences from the reference: one word wepp_pack_read_word(position, ref_nuc,
 * mut_nuc, 0) per position where the deepest mutation on the node's root path leaves mut_nuc != ref_nuc, ascending by
 * position.  d(a, b) = the number of positions at which the two lists differ, "no entry" being a value of its own:
 * masks are compared for equality (an ambiguous mask or 15 is one more value), two different alleles at one position
 * count 1, d is symmetric; it is the Hamming distance of the vectors of 4-bit masks with "no entry" written 0000.
 * keep_bits (or NULL: every position is kept) restricts both lists first, as print_mutation_distance does with
 * site_read_map: position p is kept when p < keep_positions and bit p & 31 of keep_bits[p / 32] is set.
 * wepp_geno_diameters: group k = the items grp_off[k] .. grp_off[k + 1]; diam[k] = the largest d of two of its items,
 *   0 for a group of 0 or 1 items.  n_groups == 0: WEPP_OK.
 * wepp_geno_nearest: items [0, n_a) are A, the rest B; min_dist[a] = the least d(a, b), nearest[a] = the lowest index
 *   into B attaining it; matrix (or NULL) receives d(a, b) at [a * n_b + b].
 * On the device every item becomes four bit-planes over the distinct kept positions of its group (of A and B
 * together); the planes of the groups are worked off in passes of consecutive groups holding at most 1 GiB of planes
 * (GENO_PASS_BYTES, wepp_amd/csrc/geno.hpp).  WEPP_GENO_PASS_BYTES in the environment (diagnostic, read once per call,
 * changes no result) lowers that bound; a single group, or A and B together, beyond 1 GiB is WEPP_ELIMIT.
 * Results are bit-identical from run to run.
 * WEPP_EINVAL: a null argument, positions of an item not strictly ascending, mut_nuc == ref_nuc or mut_nuc == 0, bits
 * above mut_nuc set, a position above WEPP_MAX_POSITION, item_off[0] / grp_off[0] != 0 or offsets that do not ascend,
 * grp_off that does not end at n_items, n_a == 0 or an empty B.  WEPP_ELIMIT besides: n_items >= 2^31, 2^32 or more
 * words, a matrix of more than 2^28 cells. */
typedef struct {
    uint32_t n_items;
    const uint64_t *item_off;    /* [n_items + 1] */
    const uint32_t *item_word;   /* wepp_pack_read_word(pos, ref, mut, 0): sorted by position, positions unique,
                                    mut != ref, mut in 1..15 */
} wepp_genotypes;
int wepp_geno_diameters(int device, const wepp_genotypes *g, const uint32_t *keep_bits, uint32_t keep_positions,
                        uint32_t n_groups, const uint32_t *grp_off /* [n_groups + 1] over the items */, int32_t *diam);
int wepp_geno_nearest(int device, const wepp_genotypes *g, uint32_t n_a, const uint32_t *keep_bits,
                      uint32_t keep_positions, int32_t *min_dist /* [n_a] */, uint32_t *nearest /* [n_a] */,
                      int32_t *matrix /* [n_a * n_b] or NULL */);
/* device time of the calling thread's last wepp_geno_diameters / wepp_geno_nearest by phase (HIP events, ms, summed
 * over the passes): the columns (keys, sort, scan); the planes; the pairs */
int wepp_geno_last_timing(double *columns_ms, double *planes_ms, double *pairs_ms);

/* ---- host-side introspection of the flattened MAT (no GPU needed) -------- *
 * Lets the CPU test-suite check the flattener (orders, parent alleles, per-node
 * constants, event stream) against the oracle.  `name` is one of: node_woff,
 * words, nkey, nstat, rank2dfs, dfs2bfs, bfs2id, dfs2id, parent_dfs, dfs_end,
 * num_leaves, blk_node0, blk_eoff, blk_sum, ev_word, ev_meta, ev_lb, cp_off, cp_word, seed_sig (the signature
 * table: rows of wepp_mat_stats::seed_chunks nibbles, 8 to a dword, padded to 16 bytes).
 * Stream fields (nkey, nstat, blk_*, ev_*, cp_*) take an optional "<i>:" prefix
 * selecting sweep stream i (default: the whole-tree stream).
 * The returned pointer is borrowed from the handle; *elem_bytes is the element
 * size and *count the number of elements. */
typedef struct wepp_flat wepp_flat_t;
int wepp_flat_create(const wepp_tree_desc *tree, wepp_flat_t **out);
int wepp_flat_get(const wepp_flat_t *flat, const char *name, const void **data, uint64_t *count,
                  uint32_t *elem_bytes);
int wepp_flat_scalars(const wepp_flat_t *flat, wepp_mat_stats *stats, uint32_t *cp_stride);
int wepp_flat_destroy(wepp_flat_t *flat);
/* The device half of wepp_mat_create on its own: uploads an image built by wepp_flat_create to HIP device `device`.
 * The image is only read, so ONE flatten serves every GPU of a node (and several handles on one GPU): the
 * multi-GPU host loop calls wepp_flat_create once and wepp_mat_upload from each device's host thread, where the
 * reference re-expands the tree per sample (src/usher_common.cpp:339).  wepp_mat_create == flatten + upload.
 * The image may be destroyed as soon as the uploads have returned. */
int wepp_mat_upload(const wepp_flat_t *flat, int device, wepp_mat_t **out);
/* The flat image as a file: one flatten per NODE when the ranks are processes of their own (one per GPU under
 * torch.distributed.run, MPI, ...): rank 0 calls wepp_flat_create + wepp_flat_save (to /dev/shm), the other ranks
 * wepp_flat_load + wepp_mat_upload -- seconds instead of a flatten each.  A cache bound to this build of the library
 * (the header pins its layout constants; WEPP_EINVAL otherwise), not an exchange format.  The file is written under
 * a temporary name and renamed: a reader never sees a partial image. */
int wepp_flat_save(const wepp_flat_t *flat, const char *path);
int wepp_flat_load(const char *path, wepp_flat_t **out);
/* Diagnostic: full flattens (wepp_mat_create, wepp_flat_create) this process has run. */
uint64_t wepp_debug_flatten_count(void);

#ifdef __cplusplus
}
#endif
#endif /* WEPP_PLACE_H */
