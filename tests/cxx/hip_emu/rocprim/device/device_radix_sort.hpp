// serial stand-in for the rocPRIM primitive resolve_kernels.hip uses (a stable sort of (key, value) pairs by bits
// [begin_bit, end_bit) of the key; see ../../hip/hip_runtime.h)
#pragma once
#include <hip/hip_runtime.h>
#include <numeric>
namespace rocprim {
template <typename K, typename V>
hipError_t radix_sort_pairs(void* temp, size_t& bytes, const K* keys_in, K* keys_out, const V* vals_in, V* vals_out, size_t n,
                            unsigned begin_bit, unsigned end_bit, hipStream_t) {
    if (!temp) { bytes = 8; return 0; }
    const K mask = end_bit - begin_bit >= sizeof(K) * 8 ? ~K(0) : (K)(((K(1) << (end_bit - begin_bit)) - 1) << begin_bit);
    std::vector<size_t> idx(n);
    std::iota(idx.begin(), idx.end(), (size_t)0);
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return (keys_in[a] & mask) < (keys_in[b] & mask); });
    for (size_t i = 0; i < n; i++) { keys_out[i] = keys_in[idx[i]]; vals_out[i] = vals_in[idx[i]]; }
    return 0;
}
}
