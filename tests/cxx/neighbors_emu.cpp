// neighbors_emu.cpp -- the kernels of wepp_epp_neighbors (wepp_amd/csrc/neighbors_kernels.hip) compiled for the host
// against tests/cxx/hip_emu and driven the way neighbors_capi.cpp drives them, on plain memory
// (tests/test_neighbors_emulation.py).  Linked with assign_emu.cpp, whose unit holds the genotype table's kernels, the
// offset scan and the emulation's globals.
#include "../../wepp_amd/csrc/neighbors_kernels.hip"
#include "../../wepp_amd/csrc/assign.hpp"
using namespace wepp;
// the passes of neighbors_capi.cpp; nbr_node / nbr_dist hold n_piv * N entries, dist (or null) [n_piv][N]
extern "C" int emu_neighbors(const uint32_t* node_woff, const uint32_t* words, const uint32_t* parent_dfs, const uint32_t* dfs_end,
                             uint32_t N, uint32_t max_pos, uint32_t K, const uint32_t* piv, uint32_t radius, int form,
                             const uint8_t* skip, uint32_t pass_cols, unsigned long long* nbr_off, uint32_t* nbr_node,
                             int32_t* nbr_dist, uint32_t* top, uint32_t* n_region, int32_t* dist) {
    NbrTree t{N, max_pos, node_woff, words, parent_dfs, dfs_end};
    const uint32_t rows = N + 1, trows = max_pos + 1, nblk = nbr_scan_blocks(rows);
    unsigned long long base = 0;
    for (uint32_t k0 = 0; k0 < K; k0 += pass_cols) {
        const uint32_t Kc = std::min(pass_cols, K - k0), Es = nbr_stride(Kc), Kp = assign_padded_cols(Kc);
        std::vector<uint8_t> geno((size_t)trows * Kp, 0); std::vector<uint16_t> pre((size_t)trows * Kp);
        std::vector<uint32_t> tb((size_t)((trows + ASG_SCAN_ROWS - 1) / ASG_SCAN_ROWS) * Kp); uint32_t flag = 0;
        launch_assign_tables(node_woff, words, parent_dfs, piv + k0, Kc, Kp, max_pos, geno.data(), pre.data(), tb.data(), &flag, nullptr);
        std::vector<int32_t> field((size_t)rows * Es, 0), over((size_t)rows * Es, 0), tover(Es);
        std::vector<uint32_t> bsum((size_t)nblk * Es), bcnt((size_t)nblk * Es), tp(Es), tend(Es), nreg(Es, 0), nlist(Es + 1, 0);
        std::vector<unsigned long long> off(Es + 1);
        launch_nbr_deltas(t, geno.data(), Kp, Es, form, field.data(), nullptr);
        launch_nbr_colscan(field.data(), Es, N, bsum.data(), nullptr);
        if (dist)
            for (uint32_t j = 0; j < Kc; j++)
                for (uint32_t n = 0; n < N; n++) dist[(size_t)(k0 + j) * N + n] = field[(size_t)n * Es + j];
        launch_nbr_over(t, field.data(), Es, radius, over.data(), nullptr);
        launch_nbr_colscan(over.data(), Es, N, bsum.data(), nullptr);
        launch_nbr_tops(t, piv + k0, Kc, field.data(), over.data(), Es, radius, tp.data(), tend.data(), tover.data(), nullptr);
        launch_nbr_count(N, over.data(), Es, tp.data(), tend.data(), tover.data(), skip, bcnt.data(), nreg.data(), nlist.data(), nullptr);
        size_t tbytes = 0; assign_scan_temp_bytes(Kc, &tbytes); char temp[16];
        launch_assign_scan(nlist.data(), off.data(), Kc, temp, tbytes, nullptr);
        launch_nbr_write(N, Kc, field.data(), over.data(), Es, tp.data(), tend.data(), tover.data(), skip, bcnt.data(), off.data(),
                         nbr_node + base, nbr_dist + base, nullptr);
        for (uint32_t j = 0; j < Kc; j++) { nbr_off[k0 + j] = base + off[j]; top[k0 + j] = tp[j]; n_region[k0 + j] = nreg[j]; }
        base += off[Kc];
    }
    nbr_off[K] = base;
    return 0;
}
