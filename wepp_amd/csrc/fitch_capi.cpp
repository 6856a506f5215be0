// fitch_capi.cpp -- C-ABI of the per-site Fitch-Sankoff pass (mapper_body,
// src/usher_mapper.cpp:7-162, driven by read_vcf(create_new_mat = true),
// src/mutation_annotated_tree.cpp:1907-2031).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <memory>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "fitch_plan.hpp"
#include "handle.hpp"
#include "staged_copy.hpp"

namespace {
thread_local double g_fitch_ms[4] = {0, 0, 0, 0};     // host preparation of the rows, uploads, kernels, sort + decode + copy-out
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// what the calling thread's last run did: the form it chose, its chunks and groups, whether a row named a node twice
thread_local int g_fitch_form = -1;
thread_local uint32_t g_fitch_chunks = 0, g_fitch_groups = 0;
thread_local int g_fitch_dups = 0;
// a test hook that is a number (fitch_plan.hpp): negative when the variable is not set
long hook_value(const char* name) { const char* env = std::getenv(name); return env ? (long)(uint32_t)std::atoi(env) : -1; }
bool hook_is_1(const char* name) { const char* env = std::getenv(name); return env && env[0] == '1'; }
}  // namespace

extern "C" int wepp_fitch_last_run_info(int* form, uint32_t* chunks, uint32_t* groups, int* duplicates_dropped) {
    if (form) *form = g_fitch_form;
    if (chunks) *chunks = g_fitch_chunks;
    if (groups) *groups = g_fitch_groups;
    if (duplicates_dropped) *duplicates_dropped = g_fitch_dups;
    return WEPP_OK;
}

extern "C" int wepp_fitch_last_timing(double* prep_ms, double* upload_ms, double* kernels_ms, double* output_ms) {
    if (prep_ms) *prep_ms = g_fitch_ms[0];
    if (upload_ms) *upload_ms = g_fitch_ms[1];
    if (kernels_ms) *kernels_ms = g_fitch_ms[2];
    if (output_ms) *output_ms = g_fitch_ms[3];
    return WEPP_OK;
}

// Everything about a tree the Fitch-Sankoff pass needs, computed and uploaded ONCE: read_vcf runs
// mapper_body row after row on one tree (src/mutation_annotated_tree.cpp:1962-2031); with a plan the
// flattening, the level / chunk tables and their device copies are not redone per call.
// The tables of a form are made by the first run that selects it (fitch_plan.hpp); each is whole or absent: a host
// table is moved in once it is built, a device table is there when its owner is not null (handle.hpp: upload_whole).
struct wepp_fitch_plan {
    int device = 0;
    FlatMAT f;
    uint32_t N = 0;
    bool sets_ok_tree = true;                  // no node has too many children for the set form's counters
    std::vector<uint32_t> meta, id2dfs, depth;
    FitchChunks chunks;                        // the two stack forms
    FitchLevelTables lv;                       // the level-synchronous form
    DevMem<uint32_t> d_meta, d_cs, d_cd, d_cm, d_co, d_lcoff, d_lpar, d_b2i, d_id2bfs, d_id2dfs;
    GrowBuf<uint8_t> d_tables;                 // the decision tables (tens of GB at 16 M nodes): grown to the largest group a run asked for
};

extern "C" int wepp_fitch_plan_create(const wepp_tree_desc* tree, int device, wepp_fitch_plan_t** out) {
    if (!tree || !out) return set_error(WEPP_EINVAL, "null argument");
    *out = nullptr;
    std::unique_ptr<wepp_fitch_plan> plan(new (std::nothrow) wepp_fitch_plan());
    if (!plan) return set_error(WEPP_ENOMEM, "out of host memory");
    plan->device = device;
    // topology only: the mutation lists of `tree` are ignored (a new MAT is being built)
    std::vector<uint32_t> zero_off((size_t)tree->n_nodes + 1, 0);
    wepp_tree_desc topo = *tree;
    topo.mut_off = zero_off.data();
    topo.mut_pos = nullptr; topo.mut_ref = nullptr; topo.mut_par = nullptr; topo.mut_mut = nullptr;
    FlatMAT& f = plan->f;
    std::string err;
    try {
        int rc = flatten_tree(topo, f, err, /*topology_only=*/true);
        if (rc != WEPP_OK) return set_error(rc, err);
    } catch (const std::bad_alloc&) {
        return set_error(WEPP_ENOMEM, "out of host memory while flattening the tree");
    }
    const uint32_t N = f.N;
    if (N >= (1u << 28)) return set_error(WEPP_ELIMIT, "more than 2^28 nodes");
    std::vector<uint32_t>&meta = plan->meta, &id2dfs = plan->id2dfs, &depth = plan->depth;
    meta.assign(N, 0); id2dfs.assign(N, 0); depth.assign(N, 0);
    std::vector<uint32_t> nchild(N, 0);
    uint32_t max_children = 0;
    for (uint32_t d = 1; d < N; d++) max_children = std::max(max_children, ++nchild[f.parent_dfs[d]]);
    // the set form of the forward pass needs non-empty allele sets (checked per row below) and 15-bit counters
    plan->sets_ok_tree = max_children <= FITCH_SETS_MAX_CHILDREN;
    for (uint32_t d = 0; d < N; d++) {
        if (d) depth[d] = depth[f.parent_dfs[d]] + 1;
        meta[d] = depth[d] | ((f.nstat[d] & NS_LEAF) ? 0x80000000u : 0u);
        id2dfs[f.dfs2id[d]] = d;
    }
    plan->N = N;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return set_error(WEPP_EDEVICE, "no HIP device available (the Fitch-Sankoff pass has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(WEPP_EINVAL, "device index out of range");
    *out = plan.release();
    return WEPP_OK;
}

extern "C" int wepp_fitch_plan_destroy(wepp_fitch_plan_t* plan) {
    if (plan) {
        (void)hipSetDevice(plan->device);
        delete plan;
    }
    return WEPP_OK;
}

namespace {

// One run on a plan: the stages below fill it in turn (wepp_fitch_plan_run lists them).
struct FitchRun {
    wepp_fitch_plan* plan = nullptr;
    // the caller's arguments
    uint32_t n_sites = 0;
    const uint8_t *site_ref = nullptr, *var_nuc = nullptr;
    const uint32_t *var_off = nullptr, *var_node = nullptr;
    uint64_t capacity = 0, *n_out = nullptr;
    uint32_t *out_site = nullptr, *out_node = nullptr;
    uint8_t *out_par = nullptr, *out_mut = nullptr;
    uint64_t nv = 0;                           // variants of all rows
    FitchForm form{};
    FitchShape shape{};
    std::vector<uint8_t> ref_idx;              // reference base index of every row
    // per-call buffers; the decision tables and the topology stay with the plan
    DevMem<uint8_t> d_ref, d_vnuc, d_vnraw, d_vnuc2;
    DevMem<uint32_t> d_voff, d_vdfs, d_vraw, d_vdfs2, d_pflags;
    DevMem<> d_inh, d_outp, d_ptmp;
    DevMem<unsigned long long> d_count; DevMem<uint2> d_out;
    // the rows as launch_fitch_prepare left them: tree samples sorted by node index (BFS for the level-synchronous
    // form, DFS for the two stack forms)
    uint32_t* keys_final = nullptr;
    uint8_t* nuc_final = nullptr;
    unsigned long long cnt = 0;                // mutations the kernels emitted
    double t_begin = 0, t_prep = 0, t_up = 0, t_kern = 0;
};

// checks 1 - 6 of a run, in the order a caller can observe: the CSR over the rows is checked before anything is sized
// from it or written through it
int check_and_choose_form(FitchRun& r) {
    if (r.var_off[0] != 0) return set_error(WEPP_EINVAL, "var_off[0] must be 0");
    for (uint32_t s = 0; s < r.n_sites; s++)
        if (r.var_off[s + 1] < r.var_off[s]) return set_error(WEPP_EINVAL, "var_off not monotone");
    r.nv = r.var_off[r.n_sites];
    if (r.nv && (!r.var_node || !r.var_nuc)) return set_error(WEPP_EINVAL, "null variant arrays");
    bool empty_set = false;                    // no base allowed: the scores leave the set forms' range
    for (uint64_t k = 0; k < r.nv; k++)
        if ((r.var_nuc[k] & 15) == 0) empty_set = true;
    // test hooks: force the score form, force the DFS stack forms
    return fitch_choose_form(r.plan->sets_ok_tree, hook_is_1("WEPP_FITCH_SCORES"), hook_is_1("WEPP_FITCH_DFS"), empty_set,
                             r.plan->f.max_depth, &r.form);
}

// check 7: the plan's host tables for the form, built by the first run that selects it (test hook: force the number of
// chunks); checks 8 and 9 with the rows' own table
int build_host_tables(FitchRun& r) {
    wepp_fitch_plan& p = *r.plan;
    if (r.form.levels) {
        if (p.lv.level_off.empty()) p.lv = fitch_build_levels(p.N, p.f.parent_dfs.data(), p.depth.data(), p.f.dfs2bfs.data());
    } else if (p.chunks.start.empty()) {
        p.chunks = fitch_build_chunks(p.N, hook_value("WEPP_FITCH_CHUNKS"), p.f.max_depth, p.f.parent_dfs.data(), p.depth.data());
    }
    r.ref_idx.resize(r.n_sites);
    for (uint32_t s = 0; s < r.n_sites; s++) {
        const uint8_t b = r.site_ref[s] & 15;
        if (b == 0 || (b & (b - 1)))
            return set_error(WEPP_EINVAL, "site_ref must be a single nucleotide (row " + std::to_string(s) + ")");
        r.ref_idx[s] = (uint8_t)__builtin_ctz(b);
    }
    if (r.nv >= (1ull << 32)) return set_error(WEPP_ELIMIT, "more than 2^32 variants in one call; split the rows");
    return WEPP_OK;
}

// check 10 and the plan's device tables for the form: those a failed run left out are made by the next
int publish_device_tables(FitchRun& r) {
    wepp_fitch_plan& p = *r.plan;
    const hipError_t e = hipSetDevice(p.device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    r.t_prep = now_ms();
    auto publish = [](DevMem<uint32_t>& dst, const std::vector<uint32_t>& src, const char* what) {
        return dst ? WEPP_OK : upload_whole(dst, src.data(), src.size(), what);
    };
    // the id map: node id -> key of the form in use (BFS index for the level-synchronous kernels, DFS index for the stack forms)
    if (r.form.levels) {
        WEPP_TRY(publish(p.d_lcoff, p.lv.coff, "level tables")); WEPP_TRY(publish(p.d_lpar, p.lv.par, "level tables"));
        if (p.d_id2bfs) return WEPP_OK;
        std::vector<uint32_t> id2bfs(p.N);
        for (uint32_t i = 0; i < p.N; i++) id2bfs[i] = p.f.dfs2bfs[p.id2dfs[i]];
        return publish(p.d_id2bfs, id2bfs, "id map");
    }
    WEPP_TRY(publish(p.d_meta, p.meta, "topology")); WEPP_TRY(publish(p.d_cs, p.chunks.start, "topology"));
    WEPP_TRY(publish(p.d_cd, p.chunks.depth, "topology")); WEPP_TRY(publish(p.d_cm, p.chunks.min, "topology"));
    WEPP_TRY(publish(p.d_co, p.chunks.open, "topology"));
    return publish(p.d_id2dfs, p.id2dfs, "id map");
}

// the shape of the run, the plan's decision tables grown to it, the per-call buffers
int shape_and_allocate(FitchRun& r) {
    wepp_fitch_plan& p = *r.plan;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    // test hook: at most this many batches per group
    r.shape = fitch_run_shape(p.N, r.n_sites, r.form.levels, p.chunks.C, p.chunks.D, free_b, p.d_tables.bytes, hook_value("WEPP_FITCH_GROUP"));
    WEPP_TRY(p.d_tables.reserve(r.shape.tables_need, SIZE_MAX, "decision tables"));       // (to the byte: no slack)
    const size_t nv = r.nv, part = r.shape.part_bytes * r.shape.group;
    WEPP_TRY(r.d_ref.alloc(r.n_sites, "rows")); WEPP_TRY(r.d_voff.alloc((size_t)r.n_sites + 1, "rows"));
    WEPP_TRY(r.d_vdfs.alloc(nv, "variants")); WEPP_TRY(r.d_vnuc.alloc(nv, "variants"));
    WEPP_TRY(r.d_vraw.alloc(nv, "variants")); WEPP_TRY(r.d_vnraw.alloc(nv, "variants"));
    WEPP_TRY(r.d_vdfs2.alloc(nv, "variants")); WEPP_TRY(r.d_vnuc2.alloc(nv, "variants"));
    WEPP_TRY(r.d_pflags.alloc(2, "row flags")); WEPP_TRY(r.d_count.alloc(1, "mutation count"));
    WEPP_TRY(r.d_inh.alloc(part, "partial sums")); WEPP_TRY(r.d_outp.alloc(part, "partial sums"));
    return r.d_out.alloc(std::max<uint64_t>(r.capacity, 1), "mutations");
}

// the rows themselves -- node ids to BFS / DFS indices, sorted per row, a node named twice keeping its later
// entry (usher_mapper.cpp:57-62) -- are prepared on the device (sort_reads.hip: launch_fitch_prepare)
int upload_and_prepare_rows(FitchRun& r) {
    const uint32_t n_sites = r.n_sites; const uint64_t nv = r.nv;
    hipError_t e = hipMemcpy(r.d_ref, r.ref_idx.data(), n_sites, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r.d_voff, r.var_off, (size_t)(n_sites + 1) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && nv) e = hipMemcpy(r.d_vraw, r.var_node, nv * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && nv) e = hipMemcpy(r.d_vnraw, r.var_nuc, nv, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(r.d_count, 0, 8);
    if (e != hipSuccess) return hip_fail(e, "upload");
    size_t ptmp = 0;
    if ((e = fitch_rows_temp_bytes(nv, n_sites, &ptmp)) != hipSuccess)
        return set_error(WEPP_ENOMEM, std::string("size of the row preparation's scratch: ") + hipGetErrorString(e));
    WEPP_TRY(r.d_ptmp.alloc(ptmp, "row preparation"));
    bool in_b = true;
    e = launch_fitch_prepare(r.d_vraw, r.d_vnraw, r.d_voff, n_sites, nv, r.plan->N, r.form.levels ? r.plan->d_id2bfs : r.plan->d_id2dfs,
                             r.d_vdfs2, r.d_vnuc2, r.d_vdfs, r.d_vnuc, r.d_pflags, r.d_ptmp, ptmp, &in_b, nullptr);
    if (e == hipErrorInvalidValue) { (void)hipGetLastError(); return set_error(WEPP_EINVAL, "var_node out of range"); }
    if (e != hipSuccess) return hip_fail(e, "preparation of the rows");
    r.keys_final = in_b ? r.d_vdfs : r.d_vdfs2;
    r.nuc_final = in_b ? r.d_vnuc : r.d_vnuc2;
    // the run is under way: from here on it is the thread's last run
    g_fitch_dups = in_b ? 0 : 1;
    g_fitch_form = r.form.levels ? WEPP_FITCH_FORM_LEVELS : r.form.sets_ok ? WEPP_FITCH_FORM_SETS : WEPP_FITCH_FORM_SCORES;
    g_fitch_chunks = r.form.levels ? 0 : r.plan->chunks.C;
    g_fitch_groups = (r.shape.nbatches + r.shape.group - 1) / r.shape.group;
    r.t_up = now_ms();
    return WEPP_OK;
}

// the kernels, a group of batches per launch, and the count of what they emitted
int run_groups(FitchRun& r) {
    wepp_fitch_plan& p = *r.plan;
    const bool sets_ok = r.form.sets_ok; const uint32_t nbatches = r.shape.nbatches, group = r.shape.group;
    const FitchLevels fl{p.N, r.form.levels ? (uint32_t)p.lv.level_off.size() - 1 : 0, p.d_lcoff, p.d_lpar};
    const FitchTree ft{p.N, p.f.max_depth, p.chunks.C, p.d_meta, p.d_cs, p.d_cd, p.d_cm, p.d_co};
    const FitchSites fs{r.n_sites, r.d_ref, r.d_voff, r.keys_final, r.nuc_final};
    hipError_t e = hipSuccess;
    for (uint32_t b0 = 0; b0 < nbatches && e == hipSuccess; b0 += group) {
        const uint32_t nb = std::min(group, nbatches - b0);
        if (r.form.levels) {
            e = launch_fitch_levels(fl, p.lv.level_off.data(), fs, b0, nb, p.d_tables, r.d_count, r.capacity, r.d_out, nullptr);
            continue;
        }
        if (sets_ok)
            e = launch_fitch_forward_sets(ft, fs, b0, nb, p.d_tables, (uint2*)r.d_inh.ptr, (uint2*)r.d_outp.ptr, nullptr);
        else
            e = launch_fitch_forward(ft, fs, b0, nb, p.d_tables, (int4*)r.d_inh.ptr, (int4*)r.d_outp.ptr, nullptr);
        if (e == hipSuccess) e = launch_fitch_backward(ft, fs, b0, nb, p.d_tables, sets_ok, r.d_count, r.capacity, r.d_out, nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(&r.cnt, r.d_count, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "Fitch-Sankoff kernels");
    r.t_kern = now_ms();
    return WEPP_OK;
}

// level form: the mutations sorted on the device -- key = row << 28 | BFS index, 28 + bits(n_sites) key bits --
// and decoded there into the caller's four arrays (the raw queue entries are dead after the key kernel: their memory
// takes the decoded rows and node ids), then copied out (staged_copy.hpp)
int emit_sorted_on_device(FitchRun& r) {
    wepp_fitch_plan& p = *r.plan;
    const unsigned long long cnt = r.cnt;
    uint32_t site_bits = 1;
    while (site_bits < 32 && (1ull << site_bits) < r.n_sites) site_bits++;
    DevMem<unsigned long long> d_k0, d_k1; DevMem<uint32_t> d_v0, d_v1;
    DevMem<> d_tmp; DevMem<uint8_t> d_pm;
    size_t tmp_bytes = 0;
    hipError_t e = sort_u64_u32_temp_bytes(cnt, 28 + site_bits, &tmp_bytes);
    if (e != hipSuccess) return hip_fail(e, "sort / decode / D2H copy of the mutations");
    WEPP_TRY(d_k0.alloc(cnt, "sort of the mutations")); WEPP_TRY(d_k1.alloc(cnt, "sort of the mutations"));
    WEPP_TRY(d_v0.alloc(cnt, "sort of the mutations")); WEPP_TRY(d_v1.alloc(cnt, "sort of the mutations"));
    WEPP_TRY(d_tmp.alloc(tmp_bytes, "sort of the mutations"));
    e = launch_fitch_sort_keys(r.d_out, cnt, d_k0, d_v0, nullptr);
    if (e == hipSuccess) e = launch_sort_u64_u32(d_k0, d_k1, d_v0, d_v1, cnt, 28 + site_bits, d_tmp, tmp_bytes, nullptr);
    if (e != hipSuccess) return hip_fail(e, "sort / decode / D2H copy of the mutations");
    uint32_t* d_site = (uint32_t*)r.d_out.ptr;
    uint32_t* d_node = d_site + cnt;
    WEPP_TRY(d_pm.alloc(cnt * 2, "decoding the mutations"));
    if (!p.d_b2i) WEPP_TRY(upload_whole(p.d_b2i, p.f.bfs2id.data(), p.N, "decoding the mutations"));
    e = launch_fitch_decode(d_k1, d_v1, p.d_b2i, cnt, d_site, d_node, d_pm, d_pm + cnt, nullptr);
    if (e == hipSuccess) e = d2h_staged(r.out_site, d_site, cnt * 4, nullptr);
    if (e == hipSuccess) e = d2h_staged(r.out_node, d_node, cnt * 4, nullptr);
    if (e == hipSuccess) e = d2h_staged(r.out_par, d_pm, cnt, nullptr);
    if (e == hipSuccess) e = d2h_staged(r.out_mut, d_pm + cnt, cnt, nullptr);
    if (e != hipSuccess) return hip_fail(e, "sort / decode / D2H copy of the mutations");
    return WEPP_OK;
}

// stack forms: rows in order; inside a row, nodes in BFS order (the order mapper_body visits them, :115) -- the
// kernels report DFS indices
int emit_sorted_on_host(FitchRun& r) {
    const FlatMAT& f = r.plan->f;
    const unsigned long long cnt = r.cnt;
    std::vector<uint2> raw(cnt);
    const hipError_t e = hipMemcpy(raw.data(), r.d_out, cnt * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "D2H copy of the mutations");
    std::vector<uint64_t> order(cnt);
    std::iota(order.begin(), order.end(), 0ull);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (raw[a].x != raw[b].x) return raw[a].x < raw[b].x;
        return f.dfs2bfs[raw[a].y & 0x0FFFFFFFu] < f.dfs2bfs[raw[b].y & 0x0FFFFFFFu];
    });
    for (uint64_t i = 0; i < cnt; i++) {
        const uint2 q = raw[order[i]];
        r.out_site[i] = q.x;
        r.out_node[i] = f.dfs2id[q.y & 0x0FFFFFFFu];
        r.out_par[i] = (uint8_t)(1u << ((q.y >> 28) & 3u));
        r.out_mut[i] = (uint8_t)(1u << ((q.y >> 30) & 3u));
    }
    return WEPP_OK;
}

int emit(FitchRun& r) {
    *r.n_out = r.cnt;
    if (r.cnt > r.capacity) return set_error(WEPP_ELIMIT, "output buffers too small: " + std::to_string(r.cnt) + " mutations");
    if (r.cnt == 0) return WEPP_OK;
    if (!r.out_site || !r.out_node || !r.out_par || !r.out_mut) return set_error(WEPP_EINVAL, "null output buffer");
    return r.form.levels ? emit_sorted_on_device(r) : emit_sorted_on_host(r);
}

}  // namespace

extern "C" int wepp_fitch_plan_run(wepp_fitch_plan_t* plan, uint32_t n_sites, const uint8_t* site_ref,
                                   const uint32_t* var_off, const uint32_t* var_node, const uint8_t* var_nuc,
                                   uint64_t capacity, uint64_t* n_out, uint32_t* out_site, uint32_t* out_node,
                                   uint8_t* out_par, uint8_t* out_mut) {
    if (!plan || !n_out || !var_off || (n_sites && !site_ref)) return set_error(WEPP_EINVAL, "null argument");
    *n_out = 0;
    if (n_sites == 0) return WEPP_OK;
    // The stages of a run.  A refused run launches nothing and leaves the thread's last run (wepp_fitch_last_run_info) as
    // it was; the four phases of wepp_fitch_last_timing -- up to hipSetDevice, through the row preparation, through the
    // read-back of the count, the rest -- are written once the kernels have finished.
    try {
        FitchRun r;
        r.plan = plan; r.n_sites = n_sites; r.site_ref = site_ref; r.var_off = var_off; r.var_node = var_node; r.var_nuc = var_nuc;
        r.capacity = capacity; r.n_out = n_out; r.out_site = out_site; r.out_node = out_node; r.out_par = out_par; r.out_mut = out_mut;
        r.t_begin = now_ms();
        WEPP_TRY(check_and_choose_form(r));
        WEPP_TRY(build_host_tables(r));
        WEPP_TRY(publish_device_tables(r));
        WEPP_TRY(shape_and_allocate(r));
        WEPP_TRY(upload_and_prepare_rows(r));
        WEPP_TRY(run_groups(r));
        const int rc = emit(r);
        g_fitch_ms[0] = r.t_prep - r.t_begin; g_fitch_ms[1] = r.t_up - r.t_prep; g_fitch_ms[2] = r.t_kern - r.t_up; g_fitch_ms[3] = now_ms() - r.t_kern;
        return rc;
    } catch (const std::bad_alloc&) {
        return set_error(WEPP_ENOMEM, "out of host memory in a Fitch-Sankoff run");
    }
}

extern "C" int wepp_fitch_sites(const wepp_tree_desc* tree, int device, uint32_t n_sites, const uint8_t* site_ref,
                                const uint32_t* var_off, const uint32_t* var_node, const uint8_t* var_nuc,
                                uint64_t capacity, uint64_t* n_out, uint32_t* out_site, uint32_t* out_node,
                                uint8_t* out_par, uint8_t* out_mut) {
    if (!tree || !n_out || !var_off || (n_sites && !site_ref)) return set_error(WEPP_EINVAL, "null argument");
    *n_out = 0;
    if (n_sites == 0) return WEPP_OK;
    wepp_fitch_plan_t* plan = nullptr;
    int rc = wepp_fitch_plan_create(tree, device, &plan);
    if (rc != WEPP_OK) return rc;
    rc = wepp_fitch_plan_run(plan, n_sites, site_ref, var_off, var_node, var_nuc, capacity, n_out, out_site, out_node, out_par,
                             out_mut);
    wepp_fitch_plan_destroy(plan);
    return rc;
}
