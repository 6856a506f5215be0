// geno_emu.cpp -- the kernels of wepp_geno_diameters / wepp_geno_nearest compiled for the host against
// tests/cxx/hip_emu, and the emulation's globals; geno_capi.cpp and errors.cpp are linked unchanged (tests/geno_emu.py).
#include "../../wepp_amd/csrc/geno_kernels.hip"
thread_local dim3 threadIdx, blockIdx; dim3 blockDim, gridDim; EmuBlock* g_blk;
alignas(16) unsigned char g_emu_lds[65536];
