// sam_host.hpp -- what the host sides of wepp_sam_build (sam_capi.cpp) and wepp_sam_build_subsampled
// (sam_subsample_capi.cpp) share: the checks of the arguments and the stages behind the keep table, written once in
// sam_capi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "epp_host.hpp"
#include "sam.hpp"

namespace wepp {

// the argument checks of wepp_sam_build, in its order: WEPP_OK, or the code with the message set
int sam_check_arguments(const uint8_t* reference, uint32_t genome_size, const wepp_sam_reads* rd, const wepp_sam_params* par, const wepp_sam_out* out);
// forgets the calling thread's last timing and pending words (every call begins with it)
void sam_reset_thread_state();

struct SamScratch {                        // blocks of R reads the stages behind the keep table work in
    uint32_t* n_words = nullptr;           // [R + 1]
    unsigned long long* word_off = nullptr;   // [R + 1]
    char* temp = nullptr;                  // max(scan_bytes, sort_bytes)
    size_t scan_bytes = 0, sort_bytes = 0;
};
int sam_get_scratch(DevPool& pool, uint32_t R, SamScratch* s);

// Word counts -> scan -> words -> sort -> heads -> groups -> merged batch of `reads` under the keep table, and every
// output of `out` (freq from d_freq).  ev holds six events: ev[0] and ev[1] have been recorded around the pile-up with
// the keep table; ev[2 .. 5] are recorded here (ev[2] first thing) and the four phases ev[0]-ev[1], ev[2]-ev[3],
// ev[3]-ev[4], ev[4]-ev[5] go to wepp_sam_last_timing.  bad_base (or null) is the pile-up's
// flag, looked at with the first wait.  With order_map, out->order[s] = order_map[the read of `reads` at place s].
int sam_finish(DevPool& pool, hipStream_t stream, const SamReadsDev& reads, uint64_t columns, const uint8_t* d_keep, const uint32_t* d_freq,
               const uint32_t* bad_base, const SamScratch& scratch, const hipEvent_t* ev, const uint32_t* order_map, wepp_sam_out* out);

}  // namespace wepp
