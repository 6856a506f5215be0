// pass2_capi.cpp -- the pass-2 entry points wepp_imputed_mutations, wepp_excess_mutations and wepp_best_nodes: host
// side of pass2_kernels.hip.  Each call lays ONE block out twice, in the handle's pinned staging buffer and in its
// grow-only device buffer (the ones wepp_place_batch uses; the calls on a handle are serial): one staged upload of the
// inputs, the kernels, the downloads through the same staging buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "handle.hpp"
#include "read_check.hpp"

namespace {

// Grow-only buffers of the handle for the pass-2 calls: `dev_bytes` of device memory in io_in and `pin_bytes`
// of pinned staging (the same buffers wepp_place_batch uses; the calls on a handle are serial).
int reserve_io(wepp_mat* mat, size_t dev_bytes, size_t pin_need) {
    WEPP_TRY(mat->io_in.reserve(dev_bytes, 4, "io buffer"));
    return mat->pin.reserve(pin_need, 4, "staging buffer");
}

// The regions of a block, one behind the other, each padded to 256 bytes: take<T>(bytes) is the next one.  The same
// sequence of calls runs over the staging base and over the device base; from a null base it only sizes (`off`).
struct Cursor {
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t bytes) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += pad256(bytes);
        return p;
    }
};

}  // namespace

extern "C" int wepp_imputed_mutations(wepp_mat_t* mat, const uint32_t* read_off, const uint32_t* read_word,
                                      uint32_t n_reads, const uint32_t* best_bfs_j, uint32_t* imp_off,
                                      int32_t* imp_pos, uint8_t* imp_nuc, uint64_t capacity) {
    if (!mat || !read_off || !best_bfs_j || !imp_off) return set_error(WEPP_EINVAL, "null argument");
    WEPP_TRY(check_read_csr(read_off, read_word, n_reads));
    std::vector<uint32_t> pairs;
    imp_off[0] = 0;
    for (uint32_t r = 0; r < n_reads; r++) {
        if (best_bfs_j[r] >= mat->dev.N) return set_error(WEPP_EINVAL, "best_bfs_j out of range");
        for (uint32_t k = read_off[r]; k < read_off[r + 1]; k++) {
            const uint32_t w = read_word[k], a = (w >> 24) & 15u;
            if (!((w >> 28) & 1u) && (a & (a - 1))) { pairs.push_back(r); pairs.push_back(k); }
        }
        imp_off[r + 1] = (uint32_t)(pairs.size() / 2);
    }
    const uint32_t np = (uint32_t)(pairs.size() / 2);
    if (np > capacity) return set_error(WEPP_ELIMIT, "imputed-mutation buffers too small: need " + std::to_string(np));
    if (np == 0) return WEPP_OK;
    if (!imp_pos || !imp_nuc) return set_error(WEPP_EINVAL, "null argument");
    for (uint32_t i = 0; i < np; i++) imp_pos[i] = (int32_t)(read_word[pairs[2 * i + 1]] & 0xFFFFFu);
    HIP_TRY(hipSetDevice(mat->device));
    // one staged upload (offsets | words | placements | pairs) and one download (nucleotides) through the
    // handle's pinned buffer; device memory from its grow-only input buffer
    const uint64_t nw = read_off[n_reads];
    struct Block { uint32_t *off, *word, *best, *pairs; size_t up; uint8_t* nuc; size_t bytes; };
    auto lay_out = [&](char* base, bool inputs_only) {
        Cursor c{base};
        Block b{};
        b.off = c.take<uint32_t>((size_t)(n_reads + 1) * 4);
        b.word = c.take<uint32_t>(std::max<size_t>(nw * 4, 16));
        b.best = c.take<uint32_t>((size_t)n_reads * 4);
        b.pairs = c.take<uint32_t>((size_t)np * 8);
        b.up = c.off;                                 // uploaded in one staged copy
        if (inputs_only) return b;                    // (the staging buffer holds no more)
        b.nuc = c.take<uint8_t>(np);
        b.bytes = c.off;
        return b;
    };
    const Block size = lay_out(nullptr, false);
    WEPP_TRY(reserve_io(mat, size.bytes, size.up));
    const Block h = lay_out((char*)mat->pin.ptr, true), d = lay_out((char*)mat->io_in.ptr, false);
    std::memcpy(h.off, read_off, (size_t)(n_reads + 1) * 4);
    if (nw) std::memcpy(h.word, read_word, nw * 4);
    std::memcpy(h.best, best_bfs_j, (size_t)n_reads * 4);
    std::memcpy(h.pairs, pairs.data(), (size_t)np * 8);
    HIP_TRY(hipMemcpy(d.off, h.off, size.up, hipMemcpyHostToDevice));
    HIP_TRY(launch_imputed(mat->dev, d.off, d.word, d.best, d.pairs, np, d.nuc, nullptr));
    hipError_t e = hipMemcpy(h.off, d.nuc, np, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "imputed-mutation kernel");
    std::memcpy(imp_nuc, h.off, np);
    return WEPP_OK;
}

extern "C" int wepp_excess_mutations(wepp_mat_t* mat, const uint32_t* read_off, const uint32_t* read_word,
                                     uint32_t n_reads, uint32_t n_pairs, const uint32_t* pair_read,
                                     const uint32_t* pair_bfs_j, uint64_t* exc_off, int32_t* exc_pos, uint8_t* exc_ref,
                                     uint8_t* exc_par, uint8_t* exc_mut, uint64_t capacity) {
    if (!mat || !read_off || !exc_off) return set_error(WEPP_EINVAL, "null argument");
    exc_off[0] = 0;
    if (n_pairs == 0) return WEPP_OK;
    if (!pair_read || !pair_bfs_j) return set_error(WEPP_EINVAL, "null argument");
    WEPP_TRY(check_read_csr(read_off, read_word, n_reads));
    for (uint32_t i = 0; i < n_pairs; i++) {
        if (pair_read[i] >= n_reads) return set_error(WEPP_EINVAL, "pair_read out of range");
        if (pair_bfs_j[i] >= mat->dev.N) return set_error(WEPP_EINVAL, "pair_bfs_j out of range");
    }
    const uint64_t nw = read_off[n_reads];
    HIP_TRY(hipSetDevice(mat->device));
    // upload (offsets | words | pair reads | pair nodes), count, size the output, emit: all through the
    // handle's grow-only device buffer and pinned staging buffer
    struct Block { uint32_t *off, *word, *pr, *pj; size_t up; uint32_t* cnt; unsigned long long* ooff; size_t fixed; uint32_t* out; };
    auto lay_out = [&](char* base, bool inputs_only) {
        Cursor c{base};
        Block b{};
        b.off = c.take<uint32_t>((size_t)(n_reads + 1) * 4);
        b.word = c.take<uint32_t>(std::max<size_t>(nw * 4, 16));
        b.pr = c.take<uint32_t>((size_t)n_pairs * 4);
        b.pj = c.take<uint32_t>((size_t)n_pairs * 4);
        b.up = c.off;                                 // uploaded in one staged copy
        if (inputs_only) return b;                    // (the staging buffer holds no more)
        b.cnt = c.take<uint32_t>((size_t)n_pairs * 4);
        b.ooff = c.take<unsigned long long>((size_t)n_pairs * 8);
        b.fixed = c.off;
        b.out = c.take<uint32_t>(0);                  // (as long as the counts say: sized once they are back)
        return b;
    };
    const Block size = lay_out(nullptr, false);
    const size_t b_ooff = pad256((size_t)n_pairs * 8);
    WEPP_TRY(reserve_io(mat, size.fixed, std::max(size.up, b_ooff)));
    // the four inputs staged and sent up, the regions of the device block behind its base of the moment
    char* hp = nullptr;
    Block d{};
    auto stage_inputs = [&]() -> int {
        hp = (char*)mat->pin.ptr;
        const Block h = lay_out(hp, true);
        std::memcpy(h.off, read_off, (size_t)(n_reads + 1) * 4);
        if (nw) std::memcpy(h.word, read_word, nw * 4);
        std::memcpy(h.pr, pair_read, (size_t)n_pairs * 4);
        std::memcpy(h.pj, pair_bfs_j, (size_t)n_pairs * 4);
        d = lay_out((char*)mat->io_in.ptr, false);
        HIP_TRY(hipMemcpy(d.off, h.off, size.up, hipMemcpyHostToDevice));
        return WEPP_OK;
    };
    WEPP_TRY(stage_inputs());
    HIP_TRY(launch_excess(mat->dev, d.off, d.word, d.pr, d.pj, n_pairs, nullptr, d.cnt, nullptr, nullptr));
    hipError_t e = hipMemcpy(hp, d.cnt, (size_t)n_pairs * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "excess-mutation count");
    uint64_t total = 0;
    {
        const uint32_t* counts = (const uint32_t*)hp;
        for (uint32_t i = 0; i < n_pairs; i++) { total += counts[i]; exc_off[i + 1] = total; }
    }
    if (total > capacity) return set_error(WEPP_ELIMIT, "excess-mutation buffers too small: need " + std::to_string(total));
    if (total == 0) return WEPP_OK;
    if (!exc_pos || !exc_ref || !exc_par || !exc_mut) return set_error(WEPP_EINVAL, "null output array");
    {
        // the device buffer may move when it grows: the inputs are uploaded again behind the new base
        const bool grows = size.fixed + pad256(total * 4) > mat->io_in.bytes;
        WEPP_TRY(reserve_io(mat, size.fixed + pad256(total * 4), std::max({size.up, b_ooff, (size_t)total * 4})));
        hp = (char*)mat->pin.ptr;
        if (grows) WEPP_TRY(stage_inputs());
    }
    {
        unsigned long long* ho = (unsigned long long*)hp;
        for (uint32_t i = 0; i < n_pairs; i++) ho[i] = exc_off[i];
        HIP_TRY(hipMemcpy(d.ooff, ho, (size_t)n_pairs * 8, hipMemcpyHostToDevice));
    }
    HIP_TRY(launch_excess(mat->dev, d.off, d.word, d.pr, d.pj, n_pairs, d.ooff, d.cnt, d.out, nullptr));
    e = hipMemcpy(hp, d.out, total * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "excess-mutation kernel");
    const uint32_t* packed = (const uint32_t*)hp;
    for (uint64_t q = 0; q < total; q++) {
        exc_pos[q] = (int32_t)(packed[q] & 0xFFFFFu);
        exc_ref[q] = (uint8_t)((packed[q] >> 20) & 15u);
        exc_par[q] = (uint8_t)((packed[q] >> 24) & 15u);
        exc_mut[q] = (uint8_t)((packed[q] >> 28) & 15u);
    }
    return WEPP_OK;
}

// best_j_vec: every optimal node of every read (usher_common.cpp:376-381, 413-446)
extern "C" int wepp_best_nodes(wepp_mat_t* mat, const uint32_t* read_off, const uint32_t* read_word, uint32_t n_reads,
                               const int32_t* score, const uint32_t* num_best, uint64_t* best_off, uint32_t* best_nodes,
                               uint64_t capacity) {
    if (!mat || !read_off || !score || !num_best || !best_off) return set_error(WEPP_EINVAL, "null argument");
    WEPP_TRY(check_read_csr(read_off, read_word, n_reads));
    best_off[0] = 0;
    for (uint32_t r = 0; r < n_reads; r++) best_off[r + 1] = best_off[r] + num_best[r];
    const uint64_t total = best_off[n_reads];
    if (total > capacity) return set_error(WEPP_ELIMIT, "best-node list too small: need " + std::to_string(total));
    if (n_reads == 0 || total == 0) return WEPP_OK;
    if (!best_nodes) return set_error(WEPP_EINVAL, "null argument");
    if (total >= (1ull << 32)) return set_error(WEPP_ELIMIT, "more than 2^32 optimal nodes in one call; split the batch");
    const uint64_t nw = read_off[n_reads];
    HIP_TRY(hipSetDevice(mat->device));
    // device buffers (grow-only io_in): offsets | words | scores | CSR offsets | cursors | routing arrays | the list
    struct Block {
        uint32_t *off, *word; int32_t* best; unsigned long long* o64; size_t up;
        uint32_t* cursor; uint8_t* plan; uint32_t* list; int32_t* root; uint32_t *slot, *jobs, *nodes; size_t bytes;
    };
    auto lay_out = [&](char* base, bool inputs_only) {
        Cursor c{base};
        Block b{};
        b.off = c.take<uint32_t>((size_t)(n_reads + 1) * 4);
        b.word = c.take<uint32_t>(std::max<size_t>(nw * 4, 16));
        b.best = c.take<int32_t>((size_t)n_reads * 4);
        b.o64 = c.take<unsigned long long>((size_t)(n_reads + 1) * 8);
        b.up = c.off;                                 // uploaded in one staged copy
        if (inputs_only) return b;                    // (the staging buffer holds no more)
        b.cursor = c.take<uint32_t>((size_t)n_reads * 4);
        b.plan = c.take<uint8_t>(n_reads);
        b.list = c.take<uint32_t>((size_t)n_reads * 4);
        b.root = c.take<int32_t>((size_t)n_reads * 4);
        b.slot = c.take<uint32_t>((size_t)n_reads * 4);
        b.jobs = c.take<uint32_t>((size_t)n_reads * 4);
        b.nodes = c.take<uint32_t>(total * 4);
        b.bytes = c.off;
        return b;
    };
    const Block size = lay_out(nullptr, false);
    WEPP_TRY(reserve_io(mat, size.bytes, std::max(size.up, (size_t)total * 4)));
    char* hp = (char*)mat->pin.ptr;
    const Block h = lay_out(hp, true), d = lay_out((char*)mat->io_in.ptr, false);
    std::memcpy(h.off, read_off, (size_t)(n_reads + 1) * 4);
    if (nw) std::memcpy(h.word, read_word, nw * 4);
    std::memcpy(h.best, score, (size_t)n_reads * 4);
    std::memcpy(h.o64, best_off, (size_t)(n_reads + 1) * 8);
    HIP_TRY(hipMemcpy(d.off, h.off, size.up, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d.cursor, 0, (size_t)n_reads * 4, nullptr));
    // the stream of every read: the routing of a placement call with the walks off.  A read inside one genome window
    // lists its nodes on the window's stream when that is the window's candidate crown (real nodes only, a few
    // thousand of them whatever the read's root score: device_mat.hpp win_n) and smaller than the tree-wide stream of
    // its theta; a whole-tree window stream folds runs of nodes into pseudo-nodes: nothing to list there
    DevMAT dm = mat->dev;
    dm.wc_windows = 0;            // (no per-read window crowns: k_scores takes one stream per launch)
    uint32_t* tier_info = mat->lane[0].d_info + mat->lane[0].info_idx * TI_WORDS;
    uint32_t* tier_info_next = mat->lane[0].d_info + (mat->lane[0].info_idx ^ 1u) * TI_WORDS;
    uint32_t* blk_counts = mat->lane[0].d_info + 2 * TI_WORDS;
    HIP_TRY(launch_route(dm, d.off, d.word, n_reads, mat->use_crowns ? 3 : 0, 0u, WALK_JOB_EVENTS | (WALK_JOB_EVENTS << 16), WALK8_ROWS, WALK16_ROWS,
                         0xFFFFFFFFu, 0u, d.jobs, d.plan, d.root, blk_counts, tier_info, d.slot, tier_info_next, d.jobs, RouteDirect{}, nullptr));
    mat->lane[0].info_idx ^= 1u;
    HIP_TRY(launch_scatter(d.plan, d.slot, n_reads, blk_counts, tier_info, d.list, false, nullptr));
    HIP_TRY(hipMemcpy(mat->lane[0].h_info, tier_info, TI_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t* info = mat->lane[0].h_info;
    const bool debug_plans = mat->tun.debug_plans;
    for (uint32_t id = 0; id < MAX_PLANS; id++) {
        const uint32_t count = info[TI_COUNT + id];
        if (!count) continue;
        const bool win = plan_class(id) == PLAN_WIN;
        if (win ? (plan_index(id) >= mat->wstreams.size() || mat->wstreams[plan_index(id)].ncnt != nullptr)
                : (plan_class(id) != PLAN_SWEEP || plan_index(id) >= mat->streams.size()))
            return set_error(WEPP_EDEVICE, "routing produced an invalid plan id");
        const DevStream& ps = win ? mat->wstreams[plan_index(id)] : mat->streams[plan_index(id)];
        if (debug_plans) {
            const Pass2Chunks ch = pass2_chunks(count, ps.NB, ps.ncp, ps.cp_stride, true);
            fprintf(stderr, "[best_nodes] %s %u: %u reads nchunks=%u bpc=%u\n", win ? "window" : "stream", plan_index(id), count, ch.nchunks, ch.bpc);
        }
        HIP_TRY(launch_best_nodes(mat->dev, ps, d.off, d.word,
                                  d.list + info[TI_OFF + id], count, d.best, d.o64, d.cursor, d.nodes, nullptr));
    }
    {
        hipError_t e = hipMemcpy(hp, d.nodes, total * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "best-node kernel");
        std::vector<uint32_t> taken(n_reads);
        e = hipMemcpy(taken.data(), d.cursor, (size_t)n_reads * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "best-node kernel");
        for (uint32_t r = 0; r < n_reads; r++)
            if (taken[r] != num_best[r])
                return set_error(WEPP_EINVAL, "read " + std::to_string(r) + ": score / num_best are not this read's placement on this tree (" +
                                              std::to_string(taken[r]) + " nodes attain the score, num_best says " + std::to_string(num_best[r]) + ")");
    }
    std::memcpy(best_nodes, hp, total * 4);
    // (the kernel fills a read's slice in the order its waves get there: ascending BFS index is the contract)
    for (uint32_t r = 0; r < n_reads; r++)
        if (num_best[r] > 1) std::sort(best_nodes + best_off[r], best_nodes + best_off[r + 1]);
    return WEPP_OK;
}
