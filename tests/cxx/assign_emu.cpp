// assign_emu.cpp -- the kernels of wepp_epp_assign (wepp_amd/csrc/assign_kernels.hip) compiled for the host against
// tests/cxx/hip_emu and driven the way assign_capi.cpp drives them, on plain memory (tests/test_assign_emulation.py).
#include "../../wepp_amd/csrc/assign_kernels.hip"
thread_local dim3 threadIdx, blockIdx; dim3 blockDim, gridDim; EmuBlock* g_blk;
alignas(16) unsigned char g_emu_lds[65536];
using namespace wepp;
// the host flow of assign_capi.cpp on plain memory
extern "C" int emu_assign(const uint32_t* node_woff, const uint32_t* words, const uint32_t* parent_dfs, uint32_t max_pos,
                          uint32_t R, const uint32_t* read_off, const uint32_t* read_word, const int32_t* start, const int32_t* end,
                          const int32_t* degree, const uint32_t* order, uint32_t genome, uint32_t K, const uint32_t* sel,
                          int32_t* min_dist, uint32_t* n_epp, unsigned long long* asg_off, uint32_t* asg_sel, uint32_t* sel_reads,
                          unsigned long long* sel_degree, uint32_t* sel_covered, uint32_t* cover) {
    const uint32_t Kp = assign_padded_cols(K), rows = max_pos + 1, nblk = (rows + ASG_SCAN_ROWS - 1) / ASG_SCAN_ROWS;
    const uint32_t cw = (genome + 31) / 32, nslabs = Kp / ASG_SLAB;
    std::vector<uint8_t> geno((size_t)rows * Kp, 0); std::vector<uint16_t> pre((size_t)rows * Kp);
    std::vector<uint32_t> bsum((size_t)nblk * Kp), nepp(R + 1, 0), sr(Kp, 0); uint32_t flag = 0;
    std::vector<unsigned long long> sd(Kp, 0), ties((size_t)R * nslabs * 4);
    launch_assign_tables(node_woff, words, parent_dfs, sel, K, Kp, max_pos, geno.data(), pre.data(), bsum.data(), &flag, nullptr);
    AssignArgs a{};
    a.R = R; a.K = K; a.Kp = Kp; a.max_pos = max_pos; a.genome_size = genome; a.cover_words = cw;
    a.geno = geno.data(); a.pre = pre.data(); a.read_off = read_off; a.read_word = read_word; a.start = start; a.end = end;
    a.degree = degree; a.order = order; a.min_dist = min_dist; a.n_epp = nepp.data(); a.ties = ties.data();
    a.sel_reads = sr.data(); a.sel_degree = sd.data(); a.cover = cover;
    memset(cover, 0, (size_t)K * cw * 4);
    launch_assign(a, nullptr);
    launch_assign_popcount(cover, K, cw, sel_covered, nullptr);
    size_t tb = 0; assign_scan_temp_bytes(R, &tb); char temp[16];
    launch_assign_scan(nepp.data(), asg_off, R, temp, tb, nullptr);
    launch_assign_lists(ties.data(), asg_off, R, Kp, asg_sel, nullptr);
    memcpy(n_epp, nepp.data(), (size_t)R * 4); memcpy(sel_reads, sr.data(), (size_t)K * 4); memcpy(sel_degree, sd.data(), (size_t)K * 8);
    return (int)flag;
}
