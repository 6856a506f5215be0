// resolve_emu.cpp -- the kernels of wepp_epp_resolve (wepp_amd/csrc/resolve_kernels.hip, with those of wepp_epp_assign
// it runs in between) compiled for the host against tests/cxx/hip_emu and driven the way resolve_capi.cpp drives them,
// on plain memory (tests/test_resolve_emulation.py).
#include "../../wepp_amd/csrc/assign_kernels.hip"
#include "../../wepp_amd/csrc/resolve_kernels.hip"
#include "../../wepp_amd/csrc/resolve_host.hpp"
thread_local dim3 threadIdx, blockIdx; dim3 blockDim, gridDim; EmuBlock* g_blk;
alignas(16) unsigned char g_emu_lds[65536];
namespace wepp { int set_error(int code, const std::string&) { return code; } }
using namespace wepp;
extern "C" uint32_t emu_res_chunk() { return RES_CHUNK; }
// the host flow of resolve_capi.cpp on plain memory; rel_read holds R * M entries.  Returns the number of relations.
extern "C" long long emu_resolve(const uint32_t* node_woff, const uint32_t* words, const uint32_t* parent_dfs, uint32_t max_pos,
                                 uint32_t R, const uint32_t* read_off, const uint32_t* read_word, const int32_t* start,
                                 const int32_t* end, const int32_t* degree, const uint32_t* order, uint32_t genome, uint32_t K,
                                 const uint32_t* sel, uint32_t M, const uint32_t* res_word, unsigned long long* rel_off,
                                 uint32_t* rel_read, uint32_t* n_covered, uint32_t* n_masked, long long* best_degree,
                                 uint32_t* best_mask, uint32_t* hap_reads, unsigned long long* hap_degree, uint32_t* n_touched) {
    if (int rc = resolve_check_residual(M, res_word, genome)) return -rc;
    const uint32_t Kp = assign_padded_cols(K), rows = max_pos + 1, nblk = (rows + ASG_SCAN_ROWS - 1) / ASG_SCAN_ROWS;
    const uint32_t nslabs = Kp / ASG_SLAB, KW = (K + 31) / 32;
    const size_t R1 = (size_t)R + 1;
    memset(rel_off, 0, ((size_t)M + 1) * 8); memset(n_covered, 0, (size_t)M * 4); memset(n_masked, 0, (size_t)M * 4);
    memset(best_degree, 0, (size_t)M * 8); memset(best_mask, 0, (size_t)M * KW * 4);
    memset(hap_reads, 0, (size_t)M * K * 4); memset(hap_degree, 0, (size_t)M * K * 8);
    *n_touched = 0;
    if (M == 0 || R == 0) return 0;
    std::vector<uint32_t> rpos, rword, ridx;
    resolve_sort_residual(M, res_word, rpos, rword, ridx);
    std::vector<uint32_t> counts(4 * R1, 0);
    std::vector<unsigned long long> scans(4 * R1);
    MarkArgs ma{};
    ma.R = R; ma.M = M; ma.res_pos = rpos.data(); ma.res_word = rword.data(); ma.res_idx = ridx.data();
    ma.read_off = read_off; ma.read_word = read_word; ma.start = start; ma.end = end; ma.degree = degree; ma.order = order;
    ma.n_rel = counts.data(); ma.n_words = counts.data() + R1; ma.touched = counts.data() + 2 * R1; ma.touched_place = counts.data() + 3 * R1;
    ma.rel_at = scans.data(); ma.word_at = scans.data() + R1; ma.compact = scans.data() + 2 * R1; ma.place_at = scans.data() + 3 * R1;
    launch_resolve_count(ma, nullptr);
    size_t tb = 0; assign_scan_temp_bytes(R, &tb); char temp[16];
    for (int i = 0; i < 4; i++) launch_assign_scan(counts.data() + i * R1, scans.data() + i * R1, R, temp, tb, nullptr);
    const unsigned long long n_rel = scans[R], W2 = scans[R1 + R];
    const uint32_t T = (uint32_t)scans[2 * R1 + R];
    if (T == 0) return 0;
    // (one element more than needed, set to a canary: a store past the end shows)
    std::vector<uint32_t> toff((size_t)T + 2, 0xDEADBEEFu), tword(W2 + 1, 0xDEADBEEFu), torder((size_t)T + 1, 0xDEADBEEFu);
    std::vector<uint32_t> key(n_rel + 1, 0xDEADBEEFu), val(n_rel + 1, 0xDEADBEEFu), key2(n_rel), val2(n_rel);
    std::vector<int32_t> tstart(T), tend(T), tdegree(T);
    ma.out_off = toff.data(); ma.out_word = tword.data(); ma.out_start = tstart.data(); ma.out_end = tend.data();
    ma.out_degree = tdegree.data(); ma.out_order = torder.data(); ma.rel_key = key.data(); ma.rel_val = val.data();
    ma.n_covered = n_covered; ma.n_masked = n_masked;
    launch_resolve_write(ma, nullptr);
    if (toff[(size_t)T + 1] != 0xDEADBEEFu || tword[W2] != 0xDEADBEEFu || torder[T] != 0xDEADBEEFu || key[n_rel] != 0xDEADBEEFu ||
        val[n_rel] != 0xDEADBEEFu || toff[T] != W2)
        return -100;
    uint32_t key_bits = 1;
    while (key_bits < 32 && (1ull << key_bits) < M) key_bits++;
    resolve_sort_temp_bytes(n_rel, key_bits, &tb);
    launch_resolve_sort(key.data(), key2.data(), val.data(), val2.data(), n_rel, key_bits, temp, tb, nullptr);
    launch_resolve_offsets(key2.data(), n_rel, M, rel_off, nullptr);
    memcpy(rel_read, val2.data(), n_rel * 4);

    std::vector<uint8_t> geno((size_t)rows * Kp, 0); std::vector<uint16_t> pre((size_t)rows * Kp);
    std::vector<uint32_t> bsum((size_t)nblk * Kp), nepp((size_t)T + 1, 0), sr(Kp, 0), cover(16, 0); uint32_t flag = 0;
    std::vector<unsigned long long> sd(Kp, 0), ties((size_t)T * nslabs * 4);
    std::vector<int32_t> md(T);
    launch_assign_tables(node_woff, words, parent_dfs, sel, K, Kp, max_pos, geno.data(), pre.data(), bsum.data(), &flag, nullptr);
    AssignArgs a{};
    a.R = T; a.K = K; a.Kp = Kp; a.max_pos = max_pos; a.genome_size = 0; a.cover_words = 0;
    a.geno = geno.data(); a.pre = pre.data(); a.read_off = toff.data(); a.read_word = tword.data(); a.start = tstart.data();
    a.end = tend.data(); a.degree = tdegree.data(); a.order = torder.data(); a.min_dist = md.data(); a.n_epp = nepp.data();
    a.ties = ties.data(); a.sel_reads = sr.data(); a.sel_degree = sd.data(); a.cover = cover.data();
    launch_assign(a, nullptr);
    for (uint32_t x : cover) if (x) return -101;

    unsigned long long longest = 0;
    for (uint32_t m = 0; m < M; m++) longest = std::max(longest, rel_off[m + 1] - rel_off[m]);
    TallyArgs ta{};
    ta.M = M; ta.K = K; ta.Kp = Kp; ta.rel_off = rel_off; ta.rel_read = val2.data(); ta.compact = ma.compact;
    ta.degree = tdegree.data(); ta.ties = ties.data(); ta.hap_reads = hap_reads; ta.hap_degree = hap_degree;
    launch_resolve_tally(ta, (longest + RES_CHUNK - 1) / RES_CHUNK, nullptr);
    launch_resolve_best(hap_reads, hap_degree, M, K, best_degree, best_mask, nullptr);
    *n_touched = T;
    return (long long)n_rel;
}
