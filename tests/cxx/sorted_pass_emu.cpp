// sorted_pass_emu.cpp -- the sorted pass of a read with more than 64 events (wepp_amd/csrc/place_dev.hpp: sorted_fill,
// sorted_build, sorted_query) compiled for the host against tests/cxx/hip_emu, one host thread per lane
// (tests/test_sorted_pass_emulation.py).  The pass uses barriers and LDS only; the wave intrinsics of the code around it
// in place_dev.hpp are declared here so that the header parses, and end the run if anything calls them.
#include <stdlib.h>
#include <hip/hip_runtime.h>
inline int __builtin_amdgcn_update_dpp(int, int, int, int, int, bool) { abort(); }
inline int __builtin_amdgcn_readlane(int, int) { abort(); }
#include "../../wepp_amd/csrc/place_dev.hpp"
thread_local dim3 threadIdx, blockIdx; dim3 blockDim, gridDim; EmuBlock* g_blk;
alignas(16) unsigned char g_emu_lds[65536];
using namespace wepp;
namespace {
// The reads [n_reads][256] x (node, end, pk), padded with (NONE, NONE, 0) from E[rd] on, one workgroup of W waves for all
// of them in turn, as wave_walk_body deals them: a read of E <= 128 takes two rows, a larger one four, and the two
// barriers of wave_walk_body's reduction separate a read from the next.  out: [n_reads][256][6].
template <uint32_t R, uint32_t W>
void one_read(uint32_t* lds, uint32_t lane, uint32_t wv, const uint32_t* node, const uint32_t* end, const uint32_t* pk, uint32_t E, uint32_t* out) {
    uint32_t bnode[R], bend[R], bpk[R];
    for (uint32_t r = 0; r < R; r++) { const uint32_t i = lane + 64 * r; bnode[r] = node[i]; bend[r] = end[i]; bpk[r] = pk[i]; }
    sorted_fill<R, W>(lds, lane, wv, bnode, bend, bpk);
    const uint32_t rows = max((E + 63) / 64, 1u);
    for (uint32_t row = wv; row < rows; row += W) {
        const uint32_t i = lane + 64 * row;
        const PairAcc a = sorted_query<64 * R>(lds, i, bnode[row], bend[row]);
        uint32_t* o = out + 6 * i;
        o[0] = (uint32_t)a.cb; o[1] = (uint32_t)a.cB; o[2] = a.T; o[3] = a.stopA; o[4] = a.stopB; o[5] = a.fl;
    }
}
template <uint32_t W>
void k_emu(const uint32_t* node, const uint32_t* end, const uint32_t* pk, const uint32_t* E, uint32_t n_reads, uint32_t* out) {
    HIP_DYNAMIC_SHARED(uint32_t, lds)
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t rd = 0; rd < n_reads; rd++) {
        const size_t o = (size_t)rd * 256;
        if (E[rd] <= 128) one_read<2, W>(lds, lane, wv, node + o, end + o, pk + o, E[rd], out + 6 * o);
        else one_read<WW_R, W>(lds, lane, wv, node + o, end + o, pk + o, E[rd], out + 6 * o);
        __syncthreads();
        __syncthreads();
    }
}
}  // namespace
extern "C" int emu_sorted_pass(uint32_t waves, const uint32_t* node, const uint32_t* end, const uint32_t* pk, const uint32_t* E, uint32_t n_reads, uint32_t* out) {
    static_assert(ww_lds_words(4) * 4 <= sizeof(g_emu_lds), "LDS of the emulation");
    memset(g_emu_lds, 0xA5, sizeof(g_emu_lds));
    if (waves == 2) emu_launch(k_emu<2>, dim3(1), dim3(128), node, end, pk, E, n_reads, out);
    else if (waves == 4) emu_launch(k_emu<4>, dim3(1), dim3(256), node, end, pk, E, n_reads, out);
    else return 1;
    return 0;
}
