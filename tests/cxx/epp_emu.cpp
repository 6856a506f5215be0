// epp_emu.cpp -- the kernels of wepp_epp_assign, wepp_epp_resolve and wepp_epp_neighbors compiled for the host against
// tests/cxx/hip_emu, and what the entry points' OWN host sides (assign_capi.cpp, resolve_capi.cpp, neighbors_capi.cpp,
// epp_host.cpp, linked unchanged) need around them: the emulation's globals, a handle over plain arrays, and the
// check that nothing was stored outside what a call asked its device blocks for (tests/epp_emu.py).
#include "../../wepp_amd/csrc/assign_kernels.hip"
#include "../../wepp_amd/csrc/resolve_kernels.hip"
#include "../../wepp_amd/csrc/neighbors_kernels.hip"
#include "../../wepp_amd/csrc/handle.hpp"
thread_local dim3 threadIdx, blockIdx; dim3 blockDim, gridDim; EmuBlock* g_blk;
alignas(16) unsigned char g_emu_lds[65536];

extern "C" uint32_t emu_res_chunk() { return RES_CHUNK; }

// a handle whose tree arrays are the caller's (FlatView's): the caller keeps them alive
extern "C" wepp_mat* emu_mat_create(const uint32_t* node_woff, const uint32_t* words, const uint32_t* parent_dfs, uint32_t N,
                                    uint32_t max_pos) {
    wepp_mat* m = new wepp_mat;
    m->dev.N = N; m->dev.max_pos = max_pos;
    m->dev.node_woff = node_woff; m->dev.words = words; m->dev.parent_dfs = parent_dfs;
    return m;
}

extern "C" void emu_mat_destroy(wepp_mat* m) { delete m; }

// 0, or 1 + the index of the first block of the handle's cache whose bytes past the most ever asked of it, or whose
// guard behind it, are no longer the fill of the emulated hipMalloc
extern "C" int emu_guard_check(const wepp_mat* m) {
    const auto& blocks = m->epp_cache.blocks;
    for (size_t b = 0; b < blocks.size(); b++) {
        const unsigned char* p = (const unsigned char*)blocks[b].ptr;
        for (size_t i = blocks[b].asked; i < blocks[b].bytes + EMU_GUARD_BYTES; i++)
            if (p[i] != (unsigned char)(EMU_FILL >> (8 * (i & 3)))) return (int)b + 1;
    }
    return 0;
}
