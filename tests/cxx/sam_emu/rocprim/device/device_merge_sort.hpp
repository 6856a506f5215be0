// serial stand-in for the rocPRIM primitive sam_kernels.hip sorts with (see ../../../hip_emu/hip/hip_runtime.h)
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
namespace rocprim {
template <typename In, typename Out, typename Cmp>
hipError_t merge_sort(void* temp, size_t& bytes, In in, Out out, size_t n, Cmp cmp, hipStream_t) {
    if (!temp) { bytes = 8; return 0; }
    for (size_t i = 0; i < n; i++) out[i] = in[i];
    std::stable_sort(out, out + n, cmp);
    return 0;
}
}
