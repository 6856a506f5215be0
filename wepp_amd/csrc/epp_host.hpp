// epp_host.hpp -- what the host sides of the WEPP entry points (epp_capi.cpp: wepp_epp_map,
// assign_capi.cpp: wepp_epp_assign, resolve_capi.cpp: wepp_epp_resolve) share: the per-call device blocks
// taken from the handle's cache, the validation of a wepp_epp_reads batch, the (start, end) order of its
// reads, and the argument checks and the genotype table of the entry points that take a selection.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "handle.hpp"

namespace wepp {

struct DevPool {                       // device allocations of one call, taken from / returned to the handle's cache
    wepp_mat_t* mat;
    std::vector<std::pair<void*, size_t>> used;
    explicit DevPool(wepp_mat_t* m) : mat(m) {}
    ~DevPool() {
        // (a call that fails half-way may still have kernels in flight on these blocks)
        (void)hipDeviceSynchronize();
        for (auto& b : used) mat->epp_cache.blocks.push_back(b);
    }
    template <typename T>
    hipError_t get(T** out, size_t n) {
        const size_t bytes = (std::max<size_t>(n * sizeof(T), 64) + 255) & ~(size_t)255;
        // the smallest cached block that holds the request without wasting more than half of itself
        size_t best = SIZE_MAX;
        auto& cache = mat->epp_cache.blocks;
        for (size_t i = 0; i < cache.size(); i++) {
            const size_t sz = cache[i].second;
            if (sz >= bytes && sz <= 2 * bytes + (1u << 20) && (best == SIZE_MAX || sz < cache[best].second)) best = i;
        }
        if (best != SIZE_MAX) {
            used.push_back(cache[best]);
            cache.erase(cache.begin() + (std::ptrdiff_t)best);
            *out = (T*)used.back().first;
            return hipSuccess;
        }
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess && !cache.empty()) {
            // out of memory with blocks of other sizes parked in the cache: release them and try again
            for (auto& b : cache) (void)hipFree(b.first);
            cache.clear();
            e = hipMalloc(&p, bytes);
        }
        if (e == hipSuccess) used.emplace_back(p, bytes);
        *out = (T*)p;
        return e;
    }
};

// the reference's preconditions on a read batch, made explicit (read_off / start / end / degree are non-null
// when n_reads > 0, read_word when there are words): WEPP_OK, or WEPP_EINVAL with the message set.
// *total_degree receives the sum of the degrees.
int epp_validate_reads(const wepp_epp_reads* rd, long long* total_degree);
// order[s] = the read at place s of the (start, end, index) order: two stable counting passes when the
// window bounds are genome positions, a comparison sort otherwise
void epp_window_order(const wepp_epp_reads* rd, std::vector<uint32_t>& order);

// The argument checks of the entry points that take a selection (assign_capi.cpp), in the order they are made:
// what can be said about the selection without the handle; the handle, the range of the indices and the read
// arrays; then (after the entry point has looked at its own outputs) genome_size, the read words and the reads'
// preconditions.  WEPP_OK, or the code with the message set.  `out` is only compared with null.
int assign_check_selection(const wepp_epp_reads* rd, const void* out, uint32_t n_sel, const uint32_t* sel);
int assign_check_handle(const wepp_mat_t* mat, const wepp_epp_reads* rd, uint32_t n_sel, const uint32_t* sel);
int assign_check_reads(const wepp_epp_reads* rd, uint32_t genome_size);

// the selection's genotype table on the device (launch_assign_tables), its blocks taken from `pool`
struct AssignTable {
    uint32_t Kp = 0, max_pos = 0;
    uint8_t* geno = nullptr;
    uint16_t* pre = nullptr;
};
// Checks the table limits, uploads sel, builds the table and waits for it; `begin` / `end` are recorded around
// the device work.  WEPP_OK, WEPP_ELIMIT (table size, 16-bit prefix counts), WEPP_ENOMEM or WEPP_EDEVICE.
int assign_build_table(wepp_mat_t* mat, DevPool& pool, uint32_t n_sel, const uint32_t* sel, hipStream_t stream,
                       hipEvent_t begin, hipEvent_t end, AssignTable* table);

}  // namespace wepp
