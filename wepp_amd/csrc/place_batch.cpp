// place_batch.cpp -- wepp_place_batch: host buffers in, host buffers out, as a pipeline of sub-batches around
// place_device (capi.cpp).  The cut of the batch and who stages / sends which offset are read_check.hpp's; what is
// here are the HIP calls, the host workers' tasks and the atomics between them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "handle_setup.hpp"
#include "host_pool.hpp"
#include "read_check.hpp"

static_assert(PIPE_MAX_SUB_BATCHES == wepp_mat::kPipeMax, "read_check.hpp caps the sub-batches at the handle's events");

namespace {
// pinned (hipHostMalloc / hipHostRegister) host memory can be the source or the target of a DMA as it stands
bool is_pinned_host(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
}  // namespace

// Host buffers in, host buffers out.  A large batch runs as a PIPELINE of sub-batches (contiguous ranges of the
// reads): the handle's host workers check the read words of sub-batch k+1 and move them into pinned staging while
// sub-batch k's words go up on one copy stream, the kernels of k-1 run on the compute stream, the results of k-2
// come down on a second copy stream and the workers move those of k-3 out to the caller's arrays.  Buffers the
// caller has pinned are used as they are (no staging pass).  The results are the ones of the unsplit call: a
// read's placement does not depend on its batch (tests/test_gpu_parity.py::test_pipeline_equals_unsplit_call).
extern "C" int wepp_place_batch(wepp_mat_t* mat, const uint32_t* read_off, const uint32_t* read_word,
                                uint32_t n_reads, uint32_t* best_bfs_j, int32_t* score, uint32_t* num_best,
                                uint32_t* flags, int32_t* per_node_scores) {
    if (!mat || !read_off) return set_error(WEPP_EINVAL, "null argument");
    if (per_node_scores && (uint64_t)n_reads * mat->dev.N > (1ull << 31))
        return set_error(WEPP_ELIMIT, "per_node_scores: n_reads * n_nodes exceeds 2^31 values; split the batch");
    if (n_reads == 0) return WEPP_OK;
    if (read_off[0] != 0) return set_error(WEPP_EINVAL, "read_off[0] must be 0");
    const uint64_t nw = read_off[n_reads];
    if (nw && !read_word) return set_error(WEPP_EINVAL, "null read_word");
    HIP_TRY(hipSetDevice(mat->device));
    // WEPP_DEBUG_TIMING=1: wall time of the call's phases to stderr
    const bool dbg_time = mat->tun.debug_timing;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };

    WEPP_TRY(create_pipeline(mat));
    // ---- buffers: grow-only, on the handle (no hipMalloc / hipFree per call) ----
    const size_t off_bytes = (((size_t)(n_reads + 1) * 4) + 255) & ~(size_t)255;
    const size_t in_need = off_bytes + std::max<size_t>(nw * 4, 16), out_need = (size_t)n_reads * 16;
    const bool in_pinned = is_pinned_host(read_off) && (nw == 0 || is_pinned_host(read_word));
    void* dst[4] = {best_bfs_j, score, num_best, flags};
    bool out_pinned[4];
    bool any_staged_out = false;
    for (int i = 0; i < 4; i++) { out_pinned[i] = dst[i] && is_pinned_host(dst[i]); any_staged_out = any_staged_out || (dst[i] && !out_pinned[i]); }
    WEPP_TRY(mat->io_in.reserve(in_need, 4, "reads of the batch"));
    WEPP_TRY(mat->io_out.reserve(out_need, 4, "results of the batch"));
    if (!in_pinned) WEPP_TRY(mat->pin.reserve(in_need, 4, "reads of the batch"));
    if (any_staged_out) WEPP_TRY(mat->pin_out.reserve(out_need, 4, "results of the batch"));
    uint32_t* const d_off = (uint32_t*)mat->io_in.ptr;
    uint32_t* const d_word = (uint32_t*)((char*)mat->io_in.ptr + off_bytes);
    uint32_t* const d_out = (uint32_t*)mat->io_out.ptr;
    uint32_t* const pin_off = in_pinned ? nullptr : (uint32_t*)mat->pin.ptr;
    uint32_t* const pin_word = in_pinned ? nullptr : (uint32_t*)((char*)mat->pin.ptr + off_bytes);
    uint32_t* const po = (uint32_t*)mat->pin_out.ptr;

    // ---- sub-batches and tasks (read_check.hpp: batch_geometry) ----
    if (n_reads >= BIG_BATCH_READS && !mat->pool) {
        // this handle's share of the host threads the process may use (affinity mask and cgroup quota, host_pool.hpp),
        // one of them being the calling thread: the handles alive now split them (8 device threads of one C++ host
        // process, or one handle per rank when every rank is a process with its own cpuset); WEPP_HOST_THREADS fixes it
        const uint32_t share = mat->tun.host_threads ? mat->tun.host_threads
                                                     : usable_host_threads() / std::max(1u, handles_alive());
        mat->pool.reset(new HostPool(std::min<uint32_t>(15, share > 1 ? share - 1 : 1)));
    }
    const BatchGeometry g = batch_geometry(n_reads, mat->pipe_sub_batches, mat->tun.pipe_sub_batches, mat->pool ? mat->pool->workers() : 0,
                                           per_node_scores != nullptr, mat->tun.pipe_min_chunks);
    const bool big = g.big;
    const uint32_t S = g.S, C = g.C, CPS = g.CPS, PS = g.PS, PO = g.PO;
    // (several sub-batches, every result array wanted and none in memory the caller pinned: one copy per sub-batch)
    const bool merged_out = S > 1 && dst[0] && dst[1] && dst[2] && dst[3] && !out_pinned[0] && !out_pinned[1] && !out_pinned[2] && !out_pinned[3];
    const uint32_t n_stage = C * PS, n_copy = any_staged_out ? S * 4 * PO : 0;

    // The reads are checked by the staging tasks (read_check.hpp: check_reads), each moving its reads into the pinned
    // staging buffer as it goes (one pass over the input); the first offending read (lowest index) is reported.
    std::vector<uint32_t> bad(n_stage, 0xFFFFFFFFu);
    std::vector<int> what(n_stage, 0);
    std::vector<std::atomic<uint32_t>> staged(C);          // staging parts of a chunk that are done
    std::vector<std::atomic<int>> launched(S);             // 0: not yet; 1: its D2H is enqueued (pipe_out[k] recorded); -1: never will be
    for (uint32_t c = 0; c < C; c++) staged[c].store(0);
    for (uint32_t k = 0; k < S; k++) launched[k].store(0);
    std::vector<hipError_t> copy_err(std::max<uint32_t>(n_copy, 1), hipSuccess);
    auto stage_task = [&](uint32_t t) {
        const uint32_t ck = t / PS;
        const StageRange r = stage_range(g, ck, t % PS);
        if (pin_off && r.off_hi > r.off_lo) std::memcpy(pin_off + r.off_lo, read_off + r.off_lo, (size_t)(r.off_hi - r.off_lo) * 4);
        if (r.read_hi > r.read_lo) check_reads(read_off, read_word, nw, r.read_lo, r.read_hi, pin_word, bad[t], what[t]);
        staged[ck].fetch_add(1, std::memory_order_release);
    };
    auto copy_task = [&](uint32_t t) {          // t in [0, n_copy): (sub-batch, array, part)
        const uint32_t k = t / (4 * PO), i = (t / PO) % 4, part = t % PO;
        if (!dst[i] || out_pinned[i]) return;
        int st;
        while ((st = launched[k].load(std::memory_order_acquire)) == 0) std::this_thread::yield();
        if (st < 0) return;
        (void)hipSetDevice(mat->device);                              // (a worker thread starts on device 0)
        copy_err[t] = hipEventSynchronize(mat->pipe_out[k * 4 + (merged_out ? 0u : i)]);  // this array of the sub-batch has landed (the next one is on the bus)
        if (copy_err[t] != hipSuccess) return;
        const size_t lo = g.sub_lo(k), hi = g.sub_lo(k + 1);
        const size_t a = lo + (hi - lo) * part / PO, b = lo + (hi - lo) * (part + 1) / PO;
        std::memcpy((uint32_t*)dst[i] + a, po + (size_t)i * n_reads + a, (b - a) * 4);
    };
    double t_launched = 0;

    // ---- the launch sequence: H2D, kernels, D2H of every sub-batch ----
    // TWO launchers when the call has several sub-batches and the pool at least two workers: this thread takes the
    // even sub-batches (lane 0), a pool worker the odd ones (lane 1).  A device call keeps its host thread until its
    // routing counters are back (place_device polls for them); on one thread the kernels of sub-batch k + 1 were only
    // enqueued once call k had returned, so the lanes never overlapped (1 M reads in 2 / 4 calls: 1.04 / 1.10 ms against
    // 1.05 in one).  Every launcher uploads its own sub-batches, the one after the next before the device call of this one.
    const bool two_launchers = g.two_launchers;
    struct Launcher { int rc = WEPP_OK; std::string msg; };
    Launcher launcher[2];
    double t_launch[wepp_mat::kPipeMax] = {};
    std::atomic<bool> rejected{false};
    bool up_ok[wepp_mat::kPipeMax] = {};
    hipError_t up_he[wepp_mat::kPipeMax] = {};
    // the words of sub-batch k go up chunk by chunk, each as soon as its reads are checked and staged (read_check.hpp:
    // upload_range says which offsets go with a chunk and which chunks' staging they need); up_ok[k] = none of its
    // reads was rejected
    auto upload = [&](uint32_t k, const Launcher& me) {
        const uint32_t* src_off = in_pinned ? read_off : pin_off;
        const uint32_t* src_word = in_pinned ? read_word : pin_word;
        hipError_t he = hipSuccess;
        bool ok = me.rc == WEPP_OK && !rejected.load(std::memory_order_acquire);
        for (uint32_t ck = k * CPS; ck < (k + 1) * CPS && ok && he == hipSuccess; ck++) {
            const UploadRange u = upload_range(g, k, ck);
            while (staged[ck].load(std::memory_order_acquire) < PS) std::this_thread::yield();
            if (u.wait_lo < ck) while (staged[u.wait_lo].load(std::memory_order_acquire) < PS) std::this_thread::yield();
            for (uint32_t t = ck * PS; t < (ck + 1) * PS && ok; t++) ok = bad[t] == 0xFFFFFFFFu;
            if (!ok) break;
            const uint32_t w0 = read_off[g.chunk_lo(ck)], w1 = read_off[g.chunk_lo(ck + 1)];
            he = hipMemcpyAsync(d_off + u.off_lo, src_off + u.off_lo, (size_t)(u.off_hi - u.off_lo) * 4, hipMemcpyHostToDevice, mat->pipe_h2d[k % wepp_mat::kLanes]);
            if (he == hipSuccess && w1 > w0)
                he = hipMemcpyAsync(d_word + w0, src_word + w0, (size_t)(w1 - w0) * 4, hipMemcpyHostToDevice, mat->pipe_h2d[k % wepp_mat::kLanes]);
        }
        if (ok && he == hipSuccess) he = hipEventRecord(mat->pipe_up[k], mat->pipe_h2d[k % wepp_mat::kLanes]);
        if (!ok) rejected.store(true, std::memory_order_release);      // nothing of a rejected batch reaches a kernel, and nothing behind it is worth placing
        up_ok[k] = ok;
        up_he[k] = he;
    };
    auto launch_from = [&](uint32_t first, uint32_t step, Launcher& me) {
        if (first >= S) return;
        (void)hipSetDevice(mat->device);                              // (a worker thread starts on device 0)
        upload(first, me);
        for (uint32_t k = first; k < S; k += step) {
            const uint32_t lo = g.sub_lo(k), hi = g.sub_lo(k + 1);
            if (k + step < S) upload(k + step, me);
            hipError_t he = up_he[k];
            if (!up_ok[k]) {
                launched[k].store(-1, std::memory_order_release);
                continue;
            }
            const uint32_t ln = k % wepp_mat::kLanes;             // (sub-batches alternate between the handle's two lanes)
            hipStream_t cs = mat->pipe_compute[ln];
            if (he == hipSuccess) he = hipStreamWaitEvent(cs, mat->pipe_up[k], 0);
            if (he == hipSuccess) {
                // (the offsets of a sub-batch index the whole call's word array: no rebasing)
                const int prc = place_device(mat, d_off + lo, d_word, hi - lo, d_out + lo, (int32_t*)(d_out + n_reads) + lo,
                                             d_out + 2 * (size_t)n_reads + lo, d_out + 3 * (size_t)n_reads + lo, cs, lo, n_reads, ln);
                if (prc != WEPP_OK) { me.rc = prc; me.msg = wepp_last_error(); launched[k].store(-1, std::memory_order_release); continue; }
            }
            if (he == hipSuccess) he = hipEventRecord(mat->pipe_done[k], cs);
            hipStream_t ds = mat->pipe_d2h[ln];
            if (he == hipSuccess) he = hipStreamWaitEvent(ds, mat->pipe_done[k], 0);
            if (merged_out) {
                // the four result arrays of the sub-batch in ONE (2-D) copy into the staging buffer, which has the device
                // buffer's layout: a copy and an event are host calls of ~5 us each, and the host's calls are what a
                // call split into sub-batches runs out of
                if (he == hipSuccess) he = hipMemcpy2DAsync(po + lo, (size_t)n_reads * 4, d_out + lo, (size_t)n_reads * 4, (size_t)(hi - lo) * 4, 4, hipMemcpyDeviceToHost, ds);
                if (he == hipSuccess) he = hipEventRecord(mat->pipe_out[k * 4], ds);
            } else
            for (int i = 0; i < 4 && he == hipSuccess; i++) {
                if (!dst[i]) continue;
                uint32_t* to = out_pinned[i] ? (uint32_t*)dst[i] : po + (size_t)i * n_reads;
                he = hipMemcpyAsync(to + lo, d_out + (size_t)i * n_reads + lo, (size_t)(hi - lo) * 4, hipMemcpyDeviceToHost, ds);
                if (he == hipSuccess) he = hipEventRecord(mat->pipe_out[k * 4 + i], ds);   // an array is moved out while the next one comes down
            }
            if (he != hipSuccess) {
                me.rc = hip_fail(he, "H2D / kernels / D2H of a sub-batch");
                me.msg = wepp_last_error();
                launched[k].store(-1, std::memory_order_release);
                continue;
            }
            launched[k].store(1, std::memory_order_release);
            if (dbg_time) t_launch[k] = since();
        }
    };
    {
        // (the sub-batches' plan ids land in one array sized for the call: grown here, before two threads would)
        if (S > 1) WEPP_TRY(ensure_plan_buffers(mat, n_reads));
        std::lock_guard<std::mutex> lk(mat->stat_mu);
        mat->plan_reads_in = 0;
        mat->last_walk_reads = 0;
        mat->last_n_reads = 0;
    }
    if (big) {
        // two rounds on the pool: the staging tasks (and the second launcher, first in line) while this thread launches;
        // the copy-out tasks once every sub-batch's copies are enqueued.  (One round of both had the workers that ran
        // out of staging tasks spin -- yield in a loop -- for their sub-batch's launch: fifteen spinning threads beside
        // the launch thread, on a container of sixteen cores, delayed the thread they were waiting for.)
        const uint32_t extra = two_launchers ? 1u : 0u;
        const std::function<void(uint32_t)> stage_only = [&](uint32_t t) {
            if (t < extra) launch_from(1, 2, launcher[1]);
            else stage_task(t - extra);
        };
        mat->pool->start(n_stage + extra, stage_only);
        launch_from(0, two_launchers ? 2 : 1, launcher[0]);
        mat->pool->finish();
        if (dbg_time) t_launched = since();
        if (n_copy) {
            const std::function<void(uint32_t)> copy_only = [&](uint32_t t) { copy_task(t); };
            mat->pool->run(n_copy, copy_only);
        }
    } else {
        for (uint32_t t = 0; t < n_stage; t++) stage_task(t);
        launch_from(0, 1, launcher[0]);
        for (uint32_t t = 0; t < n_copy; t++) copy_task(t);
    }
    int rc = launcher[0].rc != WEPP_OK ? launcher[0].rc : launcher[1].rc;
    std::string rc_msg = launcher[0].rc != WEPP_OK ? launcher[0].msg : launcher[1].msg;
    // everything this call put on the handle's streams has finished before it returns -- also after an error, and
    // when no result array was asked for (the staging buffers belong to the next call then)
    {
        hipError_t se = hipSuccess;
        for (hipStream_t st : {mat->pipe_d2h[0], mat->pipe_d2h[1], mat->pipe_compute[0], mat->pipe_compute[1], mat->pipe_h2d[0], mat->pipe_h2d[1]}) {
            const hipError_t r = hipStreamSynchronize(st);
            if (se == hipSuccess) se = r;
        }
        if (se != hipSuccess && rc == WEPP_OK) { rc = hip_fail(se, "placement kernels / copies"); rc_msg = wepp_last_error(); }
    }
    for (uint32_t t = 0; t < n_stage; t++) {
        if (bad[t] == 0xFFFFFFFFu) continue;
        if (what[t] == 0) return set_error(WEPP_EINVAL, "read_off not monotone");
        if (what[t] == 1)
            return set_error(WEPP_EINVAL, "read " + std::to_string(bad[t]) + ": entries must be sorted by position with unique positions");
        return set_error(WEPP_EINVAL, "read " + std::to_string(bad[t]) + ": zero nucleotide mask");
    }
    if (rc != WEPP_OK) return set_error(rc, rc_msg);
    for (uint32_t t = 0; t < n_copy; t++)
        if (copy_err[t] != hipSuccess) return hip_fail(copy_err[t], "D2H copy of the results");
    if (per_node_scores) {
        DevMem<int32_t> d_pns;
        const size_t nb = (size_t)n_reads * mat->dev.N * sizeof(int32_t);
        WEPP_TRY(d_pns.alloc((size_t)n_reads * mat->dev.N, "per_node_scores"));
        if (mat->tun.debug_plans) {
            const DevStream& full = mat->streams.back();
            const Pass2Chunks ch = pass2_chunks(n_reads, full.NB, full.ncp, full.cp_stride, false);
            fprintf(stderr, "[scores] n_reads=%u nchunks=%u bpc=%u\n", n_reads, ch.nchunks, ch.bpc);
        }
        hipError_t e = launch_scores(mat->dev, mat->streams.back(), d_off, d_word, n_reads, d_pns, nullptr);   // (everything above has been synchronised)
        if (e == hipSuccess) e = hipMemcpy(per_node_scores, d_pns, nb, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "per-node score kernel");
    }
    if (dbg_time) {
        fprintf(stderr, "[place_batch] %u reads in %u sub-batches (%s in, %s out): D2H of sub-batch k enqueued at", n_reads, S,
                in_pinned ? "caller-pinned" : "staged", any_staged_out ? "staged" : "caller-pinned");
        for (uint32_t k = 0; k < S; k++) fprintf(stderr, " %.3f", t_launch[k]);
        fprintf(stderr, " ms; every launch enqueued at %.3f ms; total %.3f ms\n", t_launched, since());
    }
    return WEPP_OK;
}
