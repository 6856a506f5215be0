// sam_emu.cpp -- the kernels of wepp_sam_build compiled for the host against tests/cxx/hip_emu, and the emulation's
// globals; sam_subsample_kernels.hip is a translation unit of its own, and sam_capi.cpp, sam_subsample_capi.cpp and
// errors.cpp are linked unchanged (tests/sam_emu.py).
#include "../../wepp_amd/csrc/sam_kernels.hip"
thread_local dim3 threadIdx, blockIdx; dim3 blockDim, gridDim; EmuBlock* g_blk;
alignas(16) unsigned char g_emu_lds[65536];
