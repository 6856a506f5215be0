// handle_setup.hpp -- making what a handle's placement calls run on (capi.cpp: upload_flat; place_batch.cpp: the
// pipeline's first call).  Apart from handle.hpp, so that the entry points which only borrow a handle do not see it;
// tests/cxx/handle_lifetime_main.cpp runs both functions against the emulated runtime.
#pragma once
#include <cstring>

#include "handle.hpp"
#include "info_wait.hpp"

namespace wepp {

// What the placement calls of a new handle run on: the walks' counters (two arrays of WALK_COUNTERS slots: loop
// iterations of the walks' waves, bytes their lanes asked memory for), every lane's routing counters, report block,
// side streams and events, the timing ring and, with seed_table_bytes > 0, the lanes' second-pass tables of k_seed.
// An early return leaves what was made to the handle's destructor.
inline int create_call_resources(wepp_mat* h, size_t seed_table_bytes) {
    HIP_TRY(hipMalloc((void**)&h->d_work.ptr, wepp_mat::D_WORK_BYTES));
    HIP_TRY(hipMemset(h->d_work, 0, wepp_mat::D_WORK_BYTES));
    for (PlaceLane& L : h->lane) {
        HIP_TRY(hipMalloc((void**)&L.d_info.ptr, (2 * TI_WORDS + ROUTE_BLOCKS * MAX_PLANS) * sizeof(uint32_t)));
        HIP_TRY(hipMemset(L.d_info, 0, 2 * TI_WORDS * sizeof(uint32_t)));
        // (the report block of k_step: the device stores into it, the host polls its last line)
        HIP_TRY(hipHostMalloc((void**)&L.h_info.ptr, info_block_words(TI_WORDS) * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped));
        memset(L.h_info, 0, info_block_words(TI_WORDS) * sizeof(uint32_t));
        HIP_TRY(hipHostGetDevicePointer((void**)&L.d_report, L.h_info, 0));
        WEPP_TRY(L.side.create(hipStreamCreateWithFlags, hipStreamDestroy, hipStreamNonBlocking));
        WEPP_TRY(L.join_ev.create(hipEventDisableTiming));
        WEPP_TRY(L.fork_ev.create(hipEventDisableTiming));
        WEPP_TRY(L.route_ev.create(hipEventDisableTiming));
        WEPP_TRY(L.info_ev.create(hipEventDisableTiming));
    }
    WEPP_TRY(h->ev0.create());
    WEPP_TRY(h->ev1.create());
    for (PlaceLane& L : h->lane)
        if (seed_table_bytes) {
            HIP_TRY(hipMalloc((void**)&L.d_seed_heavy.ptr, seed_table_bytes));
            HIP_TRY(hipMemset(L.d_seed_heavy, 0, seed_table_bytes));
        }
    return WEPP_OK;
}

// the streams and events of wepp_place_batch's pipeline, made by the handle's first call (and, had that failed half-way, completed by the next)
inline int create_pipeline(wepp_mat* h) {
    WEPP_TRY(h->pipe_h2d.create(hipStreamCreateWithFlags, hipStreamDestroy, hipStreamNonBlocking));
    WEPP_TRY(h->pipe_compute.create(hipStreamCreateWithFlags, hipStreamDestroy, hipStreamNonBlocking));
    WEPP_TRY(h->pipe_d2h.create(hipStreamCreateWithFlags, hipStreamDestroy, hipStreamNonBlocking));
    WEPP_TRY(h->pipe_up.create(hipEventDisableTiming));
    WEPP_TRY(h->pipe_done.create(hipEventDisableTiming));
    return h->pipe_out.create(hipEventDisableTiming);
}

}  // namespace wepp
