// serial stand-in for the rocPRIM primitive assign_kernels.hip uses (see ../../hip/hip_runtime.h)
#pragma once
#include <hip/hip_runtime.h>
namespace rocprim {
template <typename T> struct plus {};
template <typename It, typename F> struct TI { It p; F f; auto operator[](size_t i) const { return f(p[i]); } };
template <typename It, typename F> TI<It, F> make_transform_iterator(It p, F f) { return TI<It, F>{p, f}; }
template <typename In, typename Out, typename I, typename Op>
hipError_t exclusive_scan(void* temp, size_t& bytes, In in, Out out, I init, size_t n, Op, hipStream_t) {
    if (!temp) { bytes = 8; return 0; }
    I run = init; for (size_t i = 0; i < n; i++) { I v = in[i]; out[i] = run; run += v; } return 0;
}
}
