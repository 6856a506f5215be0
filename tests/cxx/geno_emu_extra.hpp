// geno_emu_extra.hpp -- what wepp_amd/csrc/geno_capi.cpp and geno_kernels.hip use of HIP beyond tests/cxx/hip_emu
// (which stays as it is): the device count and a 64-bit atomicMin.  tests/geno_emu.py puts it in front of both
// translation units with -include.
#pragma once
#include <hip/hip_runtime.h>
inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return 0; }
template <typename T> inline T atomicMin(T* p, T v) { T o = __atomic_load_n(p, __ATOMIC_RELAXED); while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} return o; }
