// capi.cpp -- extern "C" shim: handle lifetime, HBM residency, launches.
//
// Replaces the per-sample body of usher_common (src/usher_common.cpp:339-446):
// the BFS expansion, the N empty vectors per sample, both tbb::parallel_for
// passes over mapper2_body and the locked argmin become one batch call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "handle_setup.hpp"
#include "info_wait.hpp"
#include "launch_plan.hpp"

namespace wepp {

size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace wepp

namespace {
// The sweep loads two events per lane from every block start and the summaries of the next three blocks without
// looking at the stream's end: a stream's event words, bounds and block summaries are appended with padding behind
// the last event / block.
void append_padded(const Stream& st, std::vector<uint32_t>& evw, std::vector<uint8_t>& evl, std::vector<BlkSum>& sums) {
    evw.insert(evw.end(), st.ev_word.begin(), st.ev_word.end());
    evw.resize(evw.size() + EV_TAIL_PAD, W_PAD);
    evl.insert(evl.end(), st.ev_lb.begin(), st.ev_lb.end());
    evl.resize(evl.size() + EV_TAIL_PAD, 255);
    sums.insert(sums.end(), st.blk_sum.begin(), st.blk_sum.end());
    sums.resize(sums.size() + SUM_TAIL_PAD, st.blk_sum.empty() ? BlkSum{} : st.blk_sum.back());
}

int up_stream(wepp_mat* h, const Stream& st, uint32_t tier, DevStream& ds) {
    ds = DevStream{};
    ds.n = st.n;
    ds.NB = st.NB;
    ds.cp_stride = st.cp_stride;
    ds.ncp = (uint32_t)st.cp_off.size() - 1;
    ds.eager = 1u;                 // (crown and window streams; the whole-tree stream clears it)
    ds.tier = tier;
    ds.e_pad = (uint32_t)st.E;
    WEPP_TRY(upload(h, st.nkey, &ds.nkey));
    WEPP_TRY(upload(h, st.nstat, &ds.nstat));
    WEPP_TRY(upload(h, st.blk_node0, &ds.blk_node0));
    WEPP_TRY(upload(h, st.blk_eoff, &ds.blk_eoff));
    WEPP_TRY(upload(h, st.ev_meta, &ds.ev_meta));
    WEPP_TRY(upload(h, st.cp_off, &ds.cp_off));
    WEPP_TRY(upload(h, st.cp_word, &ds.cp_word));
    if (!st.ncnt.empty()) WEPP_TRY(upload(h, st.ncnt, &ds.ncnt));
    std::vector<uint32_t> evw;
    std::vector<uint8_t> evl;
    std::vector<BlkSum> sums;
    append_padded(st, evw, evl, sums);
    WEPP_TRY(upload(h, evw, &ds.ev_word));
    WEPP_TRY(upload(h, evl, &ds.ev_lb));
    return upload(h, sums, &ds.blk_sum);
}

// ---- the WALK ARENA: the walk structures (position index, range-query tables) of every stream -- the window crowns
// first, then the tree-wide streams -- slice by slice in ONE allocation per array (device_mat.hpp: WcInfo = the
// offsets of a stream's slices; entry indices are absolute in the arena).  Which stream a read walks is a per-READ
// value (k_route: wsid), so one launch of k_walk serves the reads of all streams, sized without a look at the routing
// counters. ----
struct ArenaOff { size_t n = 0, ent = 0, head = 0, nest = 0, sp = 0, dst = 0; };   // elements in front of a slice, array by array (nrec, rq_pre and rq_suf share n)
struct ArenaSlice {
    const Stream* st;
    size_t info;                   // its WcInfo
    DevWalk* view;                 // a tree-wide stream's own DevWalk (null: a window crown)
};

WcInfo slice_info(const FlatMAT& f, const Stream& st, const ArenaOff& o) {
    WcInfo wi{};
    wi.n = st.n;
    wi.rq_blocks = st.rq_blocks;
    wi.last_ent = (uint32_t)(o.ent + st.ix_ent.size() - 1);
    wi.has_pre = st.ix_pre.empty() ? 0u : st.ix_pre[0];
    wi.node_off = (uint32_t)o.n;
    wi.head_off = (uint32_t)o.head;
    wi.nest_off = (uint32_t)o.nest;
    wi.dst_off = (uint32_t)o.dst;
    wi.sp_off = o.sp;
    wi.tau = st.tau;
    wi.whole = st.whole;
    wi.whole_bfs = f.rank2bfs[st.whole.rank < f.N ? st.whole.rank : 0u];
    return wi;
}

template <typename T>
hipError_t copy_slice(T* dst, const std::vector<T>& v) {
    return v.empty() ? hipSuccess : hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

int build_walk_arena(const FlatMAT& f, wepp_mat* h) {
    DevMAT& d = h->dev;
    const size_t n_wc = f.wcrowns.size() * WC_MAX;
    std::vector<ArenaSlice> slices;
    for (size_t w = 0; w < f.wcrowns.size(); w++)
        for (size_t i = 0; i < f.wcrowns[w].size(); i++) slices.push_back(ArenaSlice{&f.wcrowns[w][i], w * WC_MAX + i, nullptr});
    for (size_t i = 0; i < f.streams.size(); i++) slices.push_back(ArenaSlice{&f.streams[i], n_wc + i, &h->walks[i]});
    ArenaOff tot;
    for (const ArenaSlice& s : slices) {
        tot.n += s.st->n; tot.ent += s.st->ix_ent.size(); tot.head += s.st->ix_head.size(); tot.sp += s.st->sp.size(); tot.dst += s.st->rq_dst.size();
    }
    if (tot.ent >= 0xFFFFFFF0ull || tot.n >= 0xFFFFFFF0ull || tot.head >= 0xFFFFFFF0ull || tot.dst >= 0xFFFFFFF0ull)
        return set_error(WEPP_ELIMIT, "the walk structures exceed 2^32 index entries");
    IxHead* g_head; IxEnt* g_ent; uint8_t *g_nest, *g_sp; NodeRec* g_nrec; SegNode *g_pre, *g_suf, *g_dst;
    uint32_t* g_rtpos;                         // k_route's word per head slot, derived from g_head and g_nest slice by slice (route_pos.hpp)
    WEPP_TRY(dev_alloc(h, tot.head, &g_head));
    WEPP_TRY(dev_alloc(h, tot.ent, &g_ent));
    WEPP_TRY(dev_alloc(h, tot.head, &g_nest));
    WEPP_TRY(dev_alloc(h, tot.sp, &g_sp));
    WEPP_TRY(dev_alloc(h, tot.n, &g_nrec));
    WEPP_TRY(dev_alloc(h, tot.n, &g_pre));
    WEPP_TRY(dev_alloc(h, tot.n, &g_suf));
    WEPP_TRY(dev_alloc(h, tot.dst, &g_dst));
    WEPP_TRY(dev_alloc(h, tot.head, &g_rtpos));
    d.rt_pos = g_rtpos;
    // every slice's arrays are copied from the image into place, its entry indices rebased by a kernel
    std::vector<WcInfo> info(n_wc + f.streams.size());
    ArenaOff o;
    for (const ArenaSlice& s : slices) {
        const Stream& st = *s.st;
        // (the window crowns' nesting bytes are packed, one fewer than heads per crown; a tree-wide stream's sit at its head offset)
        if (s.view) o.nest = o.head;
        const WcInfo& wi = info[s.info] = slice_info(f, st, o);
        HIP_TRY(copy_slice(g_head + o.head, st.ix_head));
        HIP_TRY(copy_slice(g_ent + o.ent, st.ix_ent));
        HIP_TRY(copy_slice(g_nest + o.nest, st.ix_nest));
        HIP_TRY(copy_slice(g_sp + o.sp, st.sp));
        HIP_TRY(copy_slice(g_nrec + o.n, st.nrec));
        HIP_TRY(copy_slice(g_pre + o.n, st.rq_pre));
        HIP_TRY(copy_slice(g_suf + o.n, st.rq_suf));
        HIP_TRY(copy_slice(g_dst + o.dst, st.rq_dst));
        if (o.ent) HIP_TRY(launch_rebase_index(g_head + o.head, (uint32_t)st.ix_head.size(), g_ent + o.ent, (uint32_t)st.ix_ent.size(), (uint32_t)o.ent, nullptr));
        HIP_TRY(launch_route_pos(g_head + o.head, g_nest + o.nest, (uint32_t)st.ix_head.size(), g_rtpos + o.head, nullptr));
        if (s.view) {
            // the stream's own view (plan-wise users: k_route, the chunked walks): entry indices are absolute, so the
            // entries are addressed from the arena's base; positions and nodes are the stream's own
            DevWalk& dw = *s.view;
            dw.n = st.n; dw.rq_blocks = st.rq_blocks; dw.last_ent = wi.last_ent; dw.has_pre = wi.has_pre; dw.whole = st.whole;
            dw.ix_head = g_head + o.head; dw.ix_ent = g_ent; dw.ix_nest = g_nest + o.nest; dw.nrec = g_nrec + o.n;
            dw.rq_pre = g_pre + o.n; dw.rq_suf = g_suf + o.n; dw.rq_dst = g_dst + o.dst; dw.sp = g_sp + o.sp;
        } else {
            h->wc_nodes += st.n;
            h->wc_count++;
        }
        o.n += st.n; o.ent += st.ix_ent.size(); o.head += st.ix_head.size(); o.nest += st.ix_nest.size(); o.sp += st.sp.size(); o.dst += st.rq_dst.size();
    }
    HIP_TRY(hipDeviceSynchronize());
    d.tw_base = (uint32_t)n_wc;
    // ... and the window crowns' sweep streams, for the reads that cannot walk (k_sweep_arena): the same kind of arena;
    // every stream keeps its own tail padding
    {
        std::vector<int64_t> s_nkey;
        std::vector<uint32_t> s_nstat, s_node0, s_eoff, s_evw, s_cpo, s_cpw;
        std::vector<uint8_t> s_meta, s_lb;
        std::vector<BlkSum> s_sum;
        struct Off { size_t nkey, node0, eoff, sum, ev, cpo, cpw; };
        std::vector<Off> offs;
        for (const auto& wc : f.wcrowns)
            for (const Stream& st : wc) {
                offs.push_back(Off{s_nkey.size(), s_node0.size(), s_eoff.size(), s_sum.size(), s_evw.size(), s_cpo.size(), s_cpw.size()});
                s_nkey.insert(s_nkey.end(), st.nkey.begin(), st.nkey.end());
                s_nstat.insert(s_nstat.end(), st.nstat.begin(), st.nstat.end());
                s_node0.insert(s_node0.end(), st.blk_node0.begin(), st.blk_node0.end());
                s_eoff.insert(s_eoff.end(), st.blk_eoff.begin(), st.blk_eoff.end());
                append_padded(st, s_evw, s_lb, s_sum);
                s_meta.insert(s_meta.end(), st.ev_meta.begin(), st.ev_meta.end());
                s_meta.resize(s_meta.size() + EV_TAIL_PAD, 0);
                s_cpo.insert(s_cpo.end(), st.cp_off.begin(), st.cp_off.end());
                s_cpw.insert(s_cpw.end(), st.cp_word.begin(), st.cp_word.end());
            }
        const int64_t* d_nkey; const uint32_t *d_nstat, *d_node0, *d_eoff, *d_evw, *d_cpo, *d_cpw;
        const uint8_t *d_meta, *d_lb; const BlkSum* d_sum;
        WEPP_TRY(upload(h, s_nkey, &d_nkey));
        WEPP_TRY(upload(h, s_nstat, &d_nstat));
        WEPP_TRY(upload(h, s_node0, &d_node0));
        WEPP_TRY(upload(h, s_eoff, &d_eoff));
        WEPP_TRY(upload(h, s_sum, &d_sum));
        WEPP_TRY(upload(h, s_evw, &d_evw));
        WEPP_TRY(upload(h, s_meta, &d_meta));
        WEPP_TRY(upload(h, s_lb, &d_lb));
        WEPP_TRY(upload(h, s_cpo, &d_cpo));
        WEPP_TRY(upload(h, s_cpw, &d_cpw));
        std::vector<DevStream> ws(n_wc, DevStream{});
        size_t k = 0;
        for (size_t w = 0; w < f.wcrowns.size(); w++)
            for (size_t i = 0; i < f.wcrowns[w].size(); i++, k++) {
                const Stream& st = f.wcrowns[w][i];
                DevStream& ds = ws[w * WC_MAX + i];
                ds.n = st.n; ds.NB = st.NB; ds.cp_stride = st.cp_stride; ds.ncp = (uint32_t)st.cp_off.size() - 1;
                ds.eager = 1u; ds.tier = WC_SLOT; ds.e_pad = (uint32_t)st.E;
                ds.nkey = d_nkey + offs[k].nkey; ds.nstat = d_nstat + offs[k].nkey;
                ds.blk_node0 = d_node0 + offs[k].node0; ds.blk_eoff = d_eoff + offs[k].eoff; ds.blk_sum = d_sum + offs[k].sum;
                ds.ev_word = d_evw + offs[k].ev; ds.ev_meta = d_meta + offs[k].ev; ds.ev_lb = d_lb + offs[k].ev;
                ds.cp_off = d_cpo + offs[k].cpo; ds.cp_word = d_cpw + offs[k].cpw;
            }
        WEPP_TRY(upload(h, ws, &d.wc_streams));
    }
    WEPP_TRY(upload(h, info, &d.wc_info));
    d.wc_windows = (uint32_t)f.wcrowns.size();
    h->stats.n_window_crowns = h->wc_count;
    h->stats.window_crown_nodes = h->wc_nodes;
    h->walks.resize(MAX_STREAMS, DevWalk{});
    DevWalk arena{};                           // (n = 0: never a stream of its own)
    arena.ix_head = g_head; arena.ix_ent = g_ent; arena.ix_nest = g_nest; arena.sp = g_sp;
    arena.nrec = g_nrec; arena.rq_pre = g_pre; arena.rq_suf = g_suf; arena.rq_dst = g_dst;
    h->walks[WC_SLOT] = arena;
    return WEPP_OK;
}

// the device half of wepp_mat_create: the flat image `f` (flatmat.hpp) copied into HBM of `device`, plus the handle's
// streams, events and counters.  The image is only read: one image serves any number of devices / handles.
int upload_flat(const FlatMAT& f, int device, wepp_mat_t** out) {
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return set_error(WEPP_EDEVICE, "no HIP device available (the placement engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(WEPP_EINVAL, "device index out of range");
    HIP_TRY(hipSetDevice(device));

    // (every error return below frees the handle with what it holds by then; the successful return lets go of it)
    std::unique_ptr<wepp_mat> owner(new (std::nothrow) wepp_mat());
    wepp_mat* const h = owner.get();
    if (!h) return set_error(WEPP_ENOMEM, "out of host memory");
    h->device = device;
    h->bfs2id = f.bfs2id;
    h->dfs2id = f.dfs2id;
    h->stats.n_nodes = f.N;
    h->stats.n_mutations = f.M;
    h->stats.n_masked = f.n_masked;
    h->stats.n_events = f.full().E;
    h->stats.n_blocks = f.full().NB;
    h->stats.n_leaves = f.n_leaves;
    h->stats.max_depth = f.max_depth;
    h->stats.max_position = f.max_pos;
    h->stats.stream_bytes = f.full().stream_bytes();
    h->stats.n_streams = (uint32_t)f.streams.size();

    DevMAT& d = h->dev;
    d.N = f.N;
    d.max_pos = f.max_pos;
    d.bm_words = 1;
    while (d.bm_words < (f.max_pos >> 5) + 1) d.bm_words <<= 1;   // power of two (k_sweep masks the index)
    d.n_streams = (uint32_t)f.streams.size();
    d.root_base = f.root_base;
    h->tun = PlaceTunables::from_env();
    d.walk_eager_nodes = h->tun.walk_eager_nodes;
    WEPP_TRY(upload(h, f.node_woff, &d.node_woff));
    WEPP_TRY(upload(h, f.words, &d.words));
    WEPP_TRY(upload(h, f.nstat, &d.nstat));
    WEPP_TRY(upload(h, f.rank2dfs, &d.rank2dfs));
    WEPP_TRY(upload(h, f.dfs2bfs, &d.dfs2bfs));
    WEPP_TRY(upload(h, f.rank2bfs, &d.rank2bfs));
    {
        std::vector<uint32_t> bfs2dfs(f.N);
        for (uint32_t k = 0; k < f.N; k++) bfs2dfs[f.dfs2bfs[k]] = k;
        WEPP_TRY(upload(h, bfs2dfs, &d.bfs2dfs));
    }
    WEPP_TRY(upload(h, f.parent_dfs, &d.parent_dfs));
    WEPP_TRY(upload(h, f.maxnest, &d.maxnest));
    WEPP_TRY(upload(h, f.epp_word, &h->epp_word));
    WEPP_TRY(upload(h, f.epp_node, &h->epp_node));
    h->epp_events = f.epp_word.size();
    for (size_t i = 0; i < f.wstreams.size(); i++) {
        DevStream ds;
        WEPP_TRY(up_stream(h, f.wstreams[i], (uint32_t)(f.streams.size() - 1), ds));
        h->wstreams.push_back(ds);
        h->wstream_bytes.push_back(f.wstreams[i].stream_bytes());
        if (i < MAX_WINDOWS) d.win_n[i] = f.wstreams[i].ncnt.empty() ? f.wstreams[i].n : 0xFFFFFFFFu;   // (pseudo-nodes: the whole tree)
        h->stats.n_window_streams++;
        h->stats.n_window_streams_crown += f.wstreams[i].ncnt.empty() ? 1u : 0u;
        h->stats.window_stream_nodes += f.wstreams[i].n;
    }
    d.n_windows = (uint32_t)f.wstreams.size();
    if (!h->wstreams.empty()) WEPP_TRY(upload(h, h->wstreams, &h->d_wstreams));
    for (size_t i = 0; i < f.streams.size(); i++) {
        const Stream& st = f.streams[i];
        DevStream ds;
        WEPP_TRY(up_stream(h, st, (uint32_t)i, ds));
        if (i + 1 == f.streams.size()) ds.eager = 0u;      // the whole tree prunes with the block minimum
        h->streams.push_back(ds);
        h->stream_bytes.push_back(st.stream_bytes());
        h->walks.push_back(DevWalk{});      // (a view into the walk arena, filled in by build_walk_arena)
        d.tau[i] = st.tau;
        h->stats.stream_tau[i] = st.tau;
        h->stats.stream_nodes[i] = st.n;
        h->stats.stream_bytes_of[i] = st.stream_bytes();
    }
    WEPP_TRY(build_walk_arena(f, h));
    WEPP_TRY(upload(h, h->walks, &d.walks));
    // k_route's routing tables: a property of the tree, built here once (device_mat.hpp: RouteTables)
    {
        const std::vector<RouteTables> blank(1);
        WEPP_TRY(upload(h, blank, &d.route_tab));
        HIP_TRY(launch_route_tables(d, const_cast<RouteTables*>(d.route_tab), nullptr));
        HIP_TRY(hipDeviceSynchronize());
    }
    // seed signatures (flatmat.hpp): whole-genome samples
    d.seed_sig = nullptr;
    d.seed_stride = d.seed_chunks = d.seed_row_words = 0;
    if (!f.seed_sig.empty()) {
        WEPP_TRY(upload(h, f.seed_sig, &d.seed_sig));
        d.seed_stride = f.seed_stride;
        d.seed_chunks = f.seed_chunks;
        d.seed_row_words = f.seed_row_words;
    }
    h->use_seeds = h->tun.seed ? 1 : 0;
    h->stats.seed_chunks = d.seed_chunks;
    h->stats.seed_chunk_blocks = d.seed_stride;
    h->stats.seed_sig_bytes = (uint64_t)f.seed_sig.size() * 4;
    h->stats.window_size = WIN_SIZE;
    h->stats.window_stride = WIN_STRIDE;
    h->stats.window_uncovered_positions = f.max_pos + 1 > MAX_WINDOWS * WIN_STRIDE ? f.max_pos + 1 - MAX_WINDOWS * WIN_STRIDE : 0;
    {
        const bool walk_on = h->tun.walk;
        // k_walk keeps an open interval as (subtree end << WALK_DELTA_BITS) | delta in one dword: a stream of
        // 2^(32 - WALK_DELTA_BITS) nodes or more is left to the sweeps (device_mat.hpp)
        h->walk_ok = 1;
        for (const Stream& st : f.streams)
            if ((uint64_t)st.n >= (1ull << (32 - WALK_DELTA_BITS))) h->walk_ok = 0;
        h->use_walk = (walk_on && h->walk_ok) ? 1 : 0;
    }
    HIP_TRY(sweep_set_max_lds(160 * 1024));
    HIP_TRY(seed_set_max_lds(160 * 1024));
    WEPP_TRY(create_call_resources(h, h->dev.seed_chunks ? seed_heavy_bytes() : 0));
    *out = owner.release();
    return WEPP_OK;
}
}  // namespace

extern "C" int wepp_mat_create(const wepp_tree_desc* tree, int device, wepp_mat_t** out) {
    if (!tree || !out) return set_error(WEPP_EINVAL, "null argument");
    *out = nullptr;
    FlatMAT f;
    std::string err;
    try {
        int rc = flatten_tree(*tree, f, err);
        if (rc != WEPP_OK) return set_error(rc, err);
    } catch (const std::bad_alloc&) {
        return set_error(WEPP_ENOMEM, "out of host memory while flattening the tree");
    }
    return upload_flat(f, device, out);
}

// One flatten per host, one upload per device: the multi-GPU host loop flattens once (wepp_flat_create) and every
// device thread uploads the same image.
extern "C" int wepp_mat_upload(const wepp_flat_t* flat, int device, wepp_mat_t** out) {
    if (!flat || !out) return set_error(WEPP_EINVAL, "null argument");
    if (flat->f.streams.empty()) return set_error(WEPP_EINVAL, "the flat image holds no sweep streams");
    return upload_flat(flat->f, device, out);
}

extern "C" int wepp_mat_destroy(wepp_mat_t* mat) {
    delete mat;
    return WEPP_OK;
}

extern "C" int wepp_mat_get_stats(const wepp_mat_t* mat, wepp_mat_stats* out) {
    if (!mat || !out) return set_error(WEPP_EINVAL, "null argument");
    *out = mat->stats;
    return WEPP_OK;
}

extern "C" int wepp_mat_bfs_order(const wepp_mat_t* mat, uint32_t* bfs_ids) {
    if (!mat || !bfs_ids) return set_error(WEPP_EINVAL, "null argument");
    std::memcpy(bfs_ids, mat->bfs2id.data(), mat->bfs2id.size() * sizeof(uint32_t));
    return WEPP_OK;
}

extern "C" int wepp_mat_set_tile_reads(wepp_mat_t* mat, uint32_t reads_per_tile) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    if (reads_per_tile < 1 || reads_per_tile > 64) return set_error(WEPP_EINVAL, "reads_per_tile must be 1..64");
    mat->tile_reads = reads_per_tile;
    return WEPP_OK;
}

extern "C" int wepp_mat_set_use_crowns(wepp_mat_t* mat, int enable) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    mat->use_crowns = enable ? 1 : 0;
    return WEPP_OK;
}

extern "C" int wepp_mat_set_use_seeds(wepp_mat_t* mat, int enable) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    mat->use_seeds = enable ? 1 : 0;
    return WEPP_OK;
}

extern "C" int wepp_mat_set_pipeline(wepp_mat_t* mat, uint32_t sub_batches) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    if (sub_batches > wepp_mat::kPipeMax) return set_error(WEPP_EINVAL, "at most 8 sub-batches");
    mat->pipe_sub_batches = sub_batches;
    return WEPP_OK;
}

extern "C" int wepp_mat_set_use_walk(wepp_mat_t* mat, int enable) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    if (enable && !mat->walk_ok)
        return set_error(WEPP_ELIMIT, "per-read walks need streams of fewer than 2^25 nodes; this tree is placed by sweeps");
    mat->use_walk = enable ? 1 : 0;
    return WEPP_OK;
}

namespace wepp {
// The placement of one batch whose reads are on the device.  plan_base / plan_total: the batch is reads
// [plan_base, plan_base + n_reads) of a call of plan_total reads (a sub-batch of wepp_place_batch's pipeline; a
// direct wepp_place_batch_device call is the whole: base 0, total n_reads) -- where its plan ids go in d_plan_of.
// the plan id and walk-slice id of every read of a call (wepp_mat_last_plans / _crowns read them back): grow-only
int ensure_plan_buffers(wepp_mat_t* mat, uint32_t plan_total) {
    WEPP_TRY(mat->d_plan_of.reserve(plan_total, 4, "plan ids"));
    return mat->d_wsid_of.reserve((size_t)plan_total * 4, 4, "plan ids");
}

// ---- one placement call: place_device() below is a sequence of stages over one PlaceCall ----
namespace {

// The fixed regions of the lane's first block (handle.hpp: PlaceLane::ws), in the order they lie there.
constexpr uint32_t N_SORTS = 5;      // sort temp of the whole-tree plan and of the four walk classes (their sorts run on different side streams)
struct LaneRegions {
    uint32_t *list, *slot_in_blk, *key_in, *key_out, *val_in;      // val_in: the sorted lists (same offsets as in `list`)
    uint32_t* job_n;                 // jobs of every read whose walk is cut into chunks (k_route)
    uint32_t *wlist[2], *wwlist;     // the plain walk classes' reads that have events in their stream (k_route appends them); reads with many events, a wave each (wave_kernels.hip)
    uint32_t *b_first, *b_clist[2], *b_jobs[2], *b_pr[2], *b_pc[2];   // the chunked classes sized blind (k_route's tables)
    int32_t *b_ps[2], *root_score;
    void* sort_tmp;
    size_t sort_temp, bytes;         // bytes of one of the N_SORTS sort regions; of the block
};

// One cursor over the regions: run from a null base it gives the block's size (bytes), run from L.ws the pointers.
LaneRegions carve_lane(void* base, uint32_t n_reads, size_t sort_temp) {
    LaneRegions r{};
    const size_t list_bytes = pad256((size_t)n_reads * 4);      // (the plan ids live in mat->d_plan_of)
    size_t off = 0;
    auto take = [&](auto*& region, size_t bytes) {
        region = reinterpret_cast<std::remove_reference_t<decltype(region)>>((uintptr_t)base + off);
        off += bytes;
    };
    take(r.list, list_bytes);
    take(r.root_score, list_bytes);
    take(r.slot_in_blk, list_bytes);
    take(r.job_n, list_bytes);
    take(r.wlist[0], list_bytes);
    take(r.wlist[1], list_bytes);
    take(r.b_first, list_bytes);
    take(r.wwlist, list_bytes);
    // (the chunked walk classes sized blind: per class its reads, its job table, three partials per job)
    for (uint32_t cc = 0; cc < 2; cc++) {
        take(r.b_clist[cc], (size_t)BLIND_CHUNKED_READS * 4);
        take(r.b_jobs[cc], (size_t)BLIND_JOB_CAP * 4);
        take(r.b_ps[cc], (size_t)BLIND_JOB_CAP * 4);
        take(r.b_pr[cc], (size_t)BLIND_JOB_CAP * 4);
        take(r.b_pc[cc], (size_t)BLIND_JOB_CAP * 4);
    }
    take(r.key_in, list_bytes);
    take(r.key_out, list_bytes);
    take(r.val_in, list_bytes);
    take(r.sort_tmp, N_SORTS * sort_temp);
    r.sort_temp = sort_temp;
    r.bytes = off;
    return r;
}

// What is decided before the first launch of a call, from the tunables and the handle's hints (choose_form).
struct CallForm {
    bool walking, step_unfused, report, ext_stamps, jobs8_blind, scatter_blind, ww_jobs;
    uint32_t report_seq, walk_limit, job_events, seed_min_hard, ev_slot;      // report_seq: the sequence number k_step reports with (report)
    uint32_t step_group, prev_walkers, lists_hint;      // k_step's lane groups and the hints they and the next expect_lists go by
    hipStream_t ps;                  // the plan stream
    hipEvent_t fork_from;
};

struct PlaceCall {
    wepp_mat_t* mat;
    PlaceLane* L;
    CallReads rd;
    CallResults out;
    uint32_t n_reads;
    hipStream_t stream;              // the caller's
    uint8_t* tier_of = nullptr;      // the plan id and the arena slice of every read: k_route writes both
    uint32_t* tier_info = nullptr;   // this call's set of the lane's counters on the device (blk_counts lies behind both sets)
    LaneRegions r{};
    CallForm f{};
    // what later stages need from earlier ones
    bool scattered = false, ev1_on_step = false;     // k_scatter of this call is queued on ps; the call's second time stamp rides on k_step's launch
    uint32_t walk_sides = 0;         // bit i: side stream i holds a walk chain, blind or late, to join into the caller's stream
};

// stage 1.  The lane's two device blocks (handle.hpp: PlaceLane).  L.ws, the fixed regions: sized by n_reads alone and
// grown here, before k_route writes into them, so they stay where they are for the whole call.  L.part, the partials:
// sized from the routing counters and grown behind the planner (reserve_partials), before anything of this call has
// touched it.
int carve_workspace(PlaceCall& c, uint32_t plan_base) {
    PlaceLane& L = *c.L;
    size_t sort_temp = 0;
    HIP_TRY(sort_reads_temp_bytes(c.n_reads, &sort_temp));
    sort_temp = pad256(sort_temp);
    // (half as much again, as ever; a device-wide synchronisation in front of the free: the lane's previous call may
    // still run out of these regions)
    WEPP_TRY(L.ws.reserve(carve_lane(nullptr, c.n_reads, sort_temp).bytes, 2, "workspace"));
    c.r = carve_lane(L.ws.ptr, c.n_reads, sort_temp);
    c.tier_of = c.mat->d_plan_of + plan_base;
    c.rd.root_score = c.r.root_score;
    c.rd.wsid = c.mat->d_wsid_of + plan_base;   // the window crown (index into DevMAT::wc_info) of every read routed to slot WC_SLOT
    c.tier_info = L.d_info + L.info_idx * TI_WORDS;
    return WEPP_OK;
}

// stage 2.  The only reader of the handle's hints before the call; it claims the call's slot of the event ring and,
// for a call by report, the lane's next sequence number.
CallForm choose_form(wepp_mat_t* mat, PlaceLane& L, uint32_t n_reads, hipStream_t stream) {
    const PlaceTunables& tun = mat->tun;
    CallForm f{};
    // events per job of the two chunked classes: they follow the handle's traffic (device_mat.hpp: WALK_TARGET_JOBS)
    f.job_events = mat->job_events[0] | (mat->job_events[1] << 16);
    // whole-genome samples are seeded (seed_kernels.hip) when work skipping is on and the tree carries signatures
    f.seed_min_hard = (mat->use_seeds && mat->use_crowns && mat->dev.seed_chunks) ? tun.seed_min_hard : 0xFFFFFFFFu;
    f.ev_slot = (uint32_t)(mat->n_timed.fetch_add(1, std::memory_order_relaxed) % wepp_mat::kRing);
    // Streams of a call (handle.hpp: SIDE_*).  The caller's stream runs k_route and, right behind it (no cross-stream wait: ~25 us), the
    // chunked walks of the first class -- the longest chain of the common case; the plain walks and the second chunked
    // class start from the routing kernel's event on side streams; everything the HOST has to size -- the counters'
    // copy, k_scatter, the sweeps, the planned walks -- lives on the plan stream `ps`, off the walks' path.  What ran
    // there behind the copy joins the caller's stream at the end; a call that launched nothing there joins nothing.
    f.walking = mat->use_walk && tun.walk_max_events;
    f.ps = f.walking ? L.side[SIDE_PLAN] : stream;
    // WEPP_STEP_UNFUSED=1 (A/B aid): the launches behind k_route as they were before k_step -- the plain walks, k_walk_wave
    // on a side stream, the 8-entry job class blind on another, forked from an event of their own; results are identical
    f.step_unfused = tun.step_unfused;
    // what the side streams of a call wait for: the event behind k_route.  The timing event of the call's ring slot is
    // recorded there anyway and serves (a second record cost a call into the runtime per step).
    f.fork_from = f.step_unfused ? (hipEvent_t)L.route_ev : mat->ev0[f.ev_slot];
    // THE COUNTERS' WAY TO THE HOST.  A call with k_step has the kernel report them: its first wave copies them into the
    // lane's block of host memory and stores this call's sequence number behind them (walk_kernels.hip), the host polls
    // that word -- no second stream, no copy, no event in front of the poll.  Every other call (walks off,
    // WEPP_STEP_UNFUSED=1) and WEPP_INFO_COPY=1 (A/B aid and fallback) copy them on the plan stream and poll an event.
    f.report = f.walking && !f.step_unfused && !tun.info_copy && n_reads > 0;
    if (f.report) f.report_seq = L.info_seq = info_next_seq(L.info_seq);
    // THE TWO TIME STAMPS ride on the kernels' own dispatch packets: ev0 is the stop event of k_route's launch, ev1 the
    // one of k_step's -- re-recorded at the end of the call when something was joined into the caller's stream behind
    // k_step.  WEPP_STAMP_RECORDS=1 (A/B aid): two records of their own, as before.  The span means the same either way.
    f.ext_stamps = !tun.stamp_records;
    // the 8-entry job class (reads with more events than a wave pass takes): launched blind behind k_route only when the
    // handle's previous call held such reads -- two launches that find nothing, a fork and a join otherwise --, else from
    // the counters like the 16-entry class.  A hint: a call it misleads launches the class late and places every read.
    f.jobs8_blind = f.step_unfused || mat->expect_jobs8.load(std::memory_order_relaxed) != 0;
    // k_scatter (the reads grouped by plan: `list`) is read by the launches the host plans and by nothing else -- sweeps,
    // window tiles, arena sweeps, seeds, the chunked classes it plans itself, and their sorts.  A sequencing run's batch
    // holds none: the kernel, a pass over every read, runs only when the counters name a consumer (launch_plan.hpp:
    // lists_needed), LATE, behind the counters' copy.  A handle whose previous call had consumers launches it BLIND behind
    // the copy, as every call did before, and loses nothing.  A hint like expect_jobs8: a call it misleads pays the late
    // launch or an idle kernel, never a result.  Bit 0 of expect_lists = expect consumers; bit 1 = the last blind launch
    // it asked for found none: the next call WITH consumers then does not set bit 0 again, so that batches of both kinds
    // in turn do not pay an idle kernel and a join in front of every other one of them.  WEPP_SCATTER_BLIND=1 (A/B aid),
    // WEPP_STEP_UNFUSED=1 and a call without walks (every read is listed, ps is the caller's stream): always blind.
    f.lists_hint = mat->expect_lists.load(std::memory_order_relaxed);
    f.scatter_blind = !f.walking || f.step_unfused || tun.scatter_blind || (f.lists_hint & 1u) != 0;
    f.ww_jobs = mat->ww_by_jobs.load(std::memory_order_relaxed) != 0;     // (the reads with 17 - 256 events: a wave each, or jobs -- by the handle's previous call)
    // (... and then reads of up to 16 events walk plainly, as before the waves: 100 000 reads with 7 - 16 events are
    // nothing to a walk launch -- its time is its longest walk -- and 0.3 ms as jobs)
    f.walk_limit = (f.ww_jobs && !tun.ww_fixed) ? std::max(tun.walk_max_events, WALK_MAX_EVENTS_BY_JOBS) : tun.walk_max_events;
    // k_step's walkers by lane groups as wide as the most events one of them can hold: 8 lanes for the default limit, 16
    // while the handle lets up to WALK_MAX_EVENTS_BY_JOBS events walk plainly; a limit beyond (WEPP_WALK_MAX_EVENTS) and
    // WEPP_STEP_GROUPS=0 keep them lane = read.  A group pass costs a wave per 64 / G walkers where lane = read costs one
    // per 64: a batch FULL of walkers (N-rich reads, bushy trees: several hundred thousand of a million) is cheaper
    // lane = read, so the form goes by the walkers of the handle's previous call (step_walkers; a hint like ww_by_jobs:
    // a call it misleads costs time, never a result)
    f.prev_walkers = mat->step_walkers.load(std::memory_order_relaxed);
    const bool few = f.prev_walkers <= STEP_GROUPS_MAX_WALKERS;
    f.step_group = (!tun.step_groups || !few || f.walk_limit > 16u) ? 0u : f.walk_limit > 8u ? 16u : 8u;
    return f;
}

hipError_t scatter(PlaceCall& c) {
    c.scattered = true;
    // (a call by report has put nothing on the plan stream yet: it forks here, in front of its first launch there)
    if (c.f.report) {
        const hipError_t e = hipStreamWaitEvent(c.f.ps, c.f.fork_from, 0);
        if (e != hipSuccess) return e;
    }
    return launch_scatter(c.tier_of, c.r.slot_in_blk, c.n_reads, c.L->d_info + 2 * TI_WORDS, c.tier_info, c.r.list, c.f.walking, c.f.ps);
}

// one walk class out of k_route's tables: the plain classes from their read lists, the chunked ones from their job tables
hipError_t blind_class(const PlaceCall& c, uint32_t cls, hipStream_t q) {
    const LaneRegions& r = c.r;
    if (cls == PLAN_WALK8 || cls == PLAN_WALK16)
        return launch_walk_blind(c.mat->dev, cls, cls == PLAN_WALK8 ? WALK8_ROWS : WALK16_ROWS, c.n_reads, r.wlist[cls], c.tier_info + TI_WCUR + cls, c.rd, c.out,
                                 c.mat->d_work, q);
    const uint32_t cc = cls - PLAN_WALKC8;
    const WalkJobs jb{0, 0, r.b_first, c.tier_info + TI_JOVER + cc, nullptr, r.job_n, r.b_ps[cc], r.b_pr[cc], r.b_pc[cc]};   // (no list: job_first and skip instead of job_off)
    return launch_walk_jobs_blind(c.mat->dev, cls, cc ? WALK16_ROWS : WALK8_ROWS, jb, r.b_jobs[cc], c.tier_info + TI_JCUR + cc, r.b_clist[cc], c.tier_info + TI_CCUR + cc,
                                  c.rd, c.out, c.mat->d_work, q);
}

// ... on side stream i, forked from the event behind k_route and joined into the caller's stream at the end of the call
hipError_t blind_side(PlaceCall& c, uint32_t cls, uint32_t i) {
    PlaceLane& L = *c.L;
    c.walk_sides |= 1u << i;
    hipError_t e = hipStreamWaitEvent(L.side[i], c.f.fork_from, 0);
    if (e == hipSuccess) e = blind_class(c, cls, L.side[i]);
    if (e == hipSuccess) e = hipEventRecord(L.join_ev[i], L.side[i]);
    return e;
}

// the counters' copy to the host on the plan stream, and the event that tells the host when it has landed
int copy_counters(const PlaceCall& c) {
    HIP_TRY(hipMemcpyAsync(c.L->h_info, c.tier_info, TI_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, c.f.ps));
    HIP_TRY(hipEventRecord(c.L->info_ev, c.f.ps));
    return WEPP_OK;
}

// stage 3.  Route the reads to streams and launch what goes blind.
int route_and_launch_blind(PlaceCall& c) {
    wepp_mat_t* mat = c.mat;
    PlaceLane& L = *c.L;
    const CallForm& f = c.f;
    const LaneRegions& r = c.r;
    const PlaceTunables& tun = mat->tun;
    const hipStream_t stream = c.stream;
    // the counters alternate between two sets: this call's set is zero (cleared at creation or by the
    // previous k_route), and this k_route clears the other one for the next call
    uint32_t* tier_info_next = L.d_info + (L.info_idx ^ 1u) * TI_WORDS;
    // k_route places the reads that have no event in their stream itself and lists the other plain walkers; their
    // walks are launched from those lists at once, sized for the worst case, on a side stream -- the routing
    // counters' trip to the host, the planning of the rarer classes and k_scatter are off their path
    RouteDirect direct{};
    if (f.walking) direct = RouteDirect{{r.wlist[0], r.wlist[1]}, {r.b_clist[0], r.b_clist[1]}, {r.b_jobs[0], r.b_jobs[1]}, r.b_first, r.wwlist,
                                        c.out.best_bfs_j, c.out.score, c.out.num_best, c.out.flags, mat->d_work, tun.walk_max_events,
                                        tun.ww_fixed ? tun.ww_block_max_small : f.ww_jobs ? 0u : 0xFFFFFFFFu, tun.ww_fixed ? tun.ww_block_max_big : f.ww_jobs ? 0u : 0xFFFFFFFFu};
    HIP_TRY(launch_route(mat->dev, c.rd.off, c.rd.word, c.n_reads, mat->use_crowns, f.walking ? f.walk_limit : 0u, f.job_events, WALK8_ROWS, WALK16_ROWS, f.seed_min_hard, tun.seed_min_nodes, r.job_n, c.tier_of, r.root_score, c.L->d_info + 2 * TI_WORDS,
                         c.tier_info, r.slot_in_blk, tier_info_next, const_cast<uint32_t*>(c.rd.wsid), direct, stream, f.ext_stamps ? mat->ev0[f.ev_slot] : nullptr));
    L.info_idx ^= 1u;
    if (!f.ext_stamps) HIP_TRY(hipEventRecord(mat->ev0[f.ev_slot], stream));        // (the timed span of a call: everything behind the routing kernel)
    if (!f.walking) {
        // (no walks: every read is listed, on the caller's stream, the counters behind the lists as ever)
        HIP_TRY(scatter(c));
        return copy_counters(c);
    }
    if (f.step_unfused) HIP_TRY(hipEventRecord(L.route_ev, stream));
    // Launched BLIND, sized for the worst case, before the routing counters are back: the plain walkers of at most
    // WALK8_K entries -- nearly every read of a sequencing run -- and the reads with many events, a wave per 64 of them
    // (place_dev.hpp), in ONE launch on the caller's stream, right behind k_route (no cross-stream wait: ~15 - 30 us):
    // k_step's workgroups take their role from k_route's counters on the device.  The chunked class (reads with even
    // more events, cut into jobs: k_route has entered them into a job table; walk + combination leave at once when
    // the class outgrew the table, TI_JOVER: the host's planned launch takes it) goes blind on a side stream when the
    // handle expects such reads.  The classes of 9 - 16 entries are launched from the same tables once the counters
    // say they hold reads (launch_late): two launches sized for a million reads that find a handful cost
    // ~20 us of workgroup dispatch each, and eight API calls per device call.
    if (f.step_unfused) {
        HIP_TRY(blind_class(c, PLAN_WALK8, stream));
        hipStream_t q = L.side[SIDE_WAVE];
        HIP_TRY(hipStreamWaitEvent(q, f.fork_from, 0));
        HIP_TRY(launch_walk_wave(mat->dev, r.wwlist, c.tier_info + TI_WWCUR, c.n_reads, c.rd, c.out, mat->d_work, q));
        HIP_TRY(hipEventRecord(L.join_ev[SIDE_WAVE], q));
        c.walk_sides |= 1u << SIDE_WAVE;
    } else {
        // (wwlist also takes the few walkers of 9 - 16 entries k_route moves there, TI_W16WAVE, whatever the hint
        // ww_by_jobs says: k_step reads the lists' cursors, and is the plain blind walk when they are empty)
        // (the walkers by lane groups or lane = read: choose_form)
        if (tun.debug_plans) fprintf(stderr, "[step] walkers by groups of %u lanes (0: lane = read); plain walkers of the previous call: %u\n", f.step_group, f.prev_walkers);
        HIP_TRY(launch_step(mat->dev, f.step_group, WALK8_ROWS, c.n_reads, r.wlist[0], c.tier_info + TI_WCUR, r.wwlist, c.tier_info + TI_WWCUR, c.rd, c.out, mat->d_work, stream,
                            f.report ? StepReport{c.tier_info, L.d_report, f.report_seq} : StepReport{nullptr, nullptr, 0u}, f.ext_stamps ? mat->ev1[f.ev_slot] : nullptr));
        c.ev1_on_step = f.ext_stamps && c.n_reads > 0;      // (no reads, no launch)
    }
    // (the job class on a stream of its own: ~10 us that would sit behind the walks on the call's longest chain)
    if (f.jobs8_blind) HIP_TRY(blind_side(c, PLAN_WALKC8, SIDE_JOBS8));
    // COUNTERS FIRST: they are final when k_route ends (k_scatter adds only TI_OFF, which the host forms itself
    // in wait_counters -- a blind k_scatter may write those words while k_step reports them).  By report, k_step has
    // them on their way as its first act and the plan stream stays empty unless k_scatter goes blind (it forks
    // itself).  By copy, the copy goes directly behind the plan stream's wait, in front of any k_scatter, and an
    // event of its own tells the host when it has landed -- whatever is queued behind it.  Either way the host
    // then returns, and enqueues the next call's k_route, while k_step still runs.
    if (!f.report) {
        HIP_TRY(hipStreamWaitEvent(f.ps, f.fork_from, 0));
        WEPP_TRY(copy_counters(c));
    }
    if (f.scatter_blind) HIP_TRY(scatter(c));
    return WEPP_OK;
}

// The wait by report: the sequence word of the report block (info_wait.hpp: spinning, then yielding, and from 2 ms on
// asking the caller's stream now and then, so that a call whose report cannot come ends with an error instead of
// waiting on)
int wait_report(const PlaceCall& c) {
    volatile const uint32_t* const word = c.L->h_info + info_seq_word(TI_WORDS);
    const hipEvent_t step_ev = c.ev1_on_step ? c.mat->ev1[c.f.ev_slot] : nullptr;
    const hipStream_t stream = c.stream;
    const auto t_poll = std::chrono::steady_clock::now();
    const InfoWaitResult w = wait_info_word(
        c.f.report_seq, [&]() { return __atomic_load_n(word, __ATOMIC_ACQUIRE); },
        [&]() {
            const hipError_t q = step_ev ? hipEventQuery(step_ev) : hipStreamQuery(stream);
            (void)hipGetLastError();
            return q == hipSuccess ? 0 : q == hipErrorNotReady ? -1 : (int)q;
        },
        [&]() { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_poll).count(); });
    if (w.what == InfoWait::stream_error) return hip_fail((hipError_t)w.error, "waiting for the routing counters");
    if (w.what == InfoWait::lost) return set_error(WEPP_EDEVICE, "internal error: k_step ended without reporting the routing counters of its call");
    return WEPP_OK;
}

// The wait by copy: the event behind it, spinning for the first 200 us (the routing kernel of a million reads takes ~45,
// behind the reads' H2D), then yielding the core between queries -- eight ranks spinning on the cores of one container
// starve their own staging workers --, and after ~2 ms (a long queue in front of this call) waiting blocking
int wait_copy(const PlaceCall& c) {
    hipError_t q = hipErrorNotReady;
    const auto t_poll = std::chrono::steady_clock::now();
    for (;;) {
        q = hipEventQuery(c.L->info_ev);
        if (q != hipErrorNotReady) break;
        const auto waited = std::chrono::steady_clock::now() - t_poll;
        if (waited > std::chrono::milliseconds(2)) break;
        if (waited > std::chrono::microseconds(200)) std::this_thread::yield();
    }
    (void)hipGetLastError();   // "not ready" is not an error: keep it out of the launchers' hipGetLastError()
    if (q != hipSuccess) HIP_TRY(hipEventSynchronize(c.L->info_ev));
    return WEPP_OK;
}

// stage 4.  The host sizes the launches from the counters, and the GPU idles until it has: poll for them (a blocking
// wait adds its wake-up, ~15 us per call, to that idle time).
int wait_counters(PlaceCall& c) {
    PlaceLane& L = *c.L;
    WEPP_TRY(c.f.report ? wait_report(c) : wait_copy(c));
    if (c.f.walking) {
        // TI_OFF = the exclusive prefix sum of TI_COUNT, and the total behind the last plan: what k_scatter writes on
        // the device, formed here because the copy no longer waits for it (the copy has landed: h_info is the host's)
        uint32_t off = 0;
        for (uint32_t t = 0; t < MAX_PLANS; t++) { L.h_info[TI_OFF + t] = off; off += L.h_info[TI_COUNT + t]; }
        L.h_info[TI_OFF + MAX_PLANS] = off;
    }
    const uint32_t* info = L.h_info;
    if (!c.mat->tun.debug_plans) return WEPP_OK;
    fprintf(stderr, "[info] counters by %s, lane %u, sequence %u\n", c.f.report ? "report" : "copy", (uint32_t)(c.L - c.mat->lane), c.f.report_seq);
    fprintf(stderr, "[route] reads=%u resolved=%u walk=%u,%u wave=%u,%u (of them walkers of 9 - 16 entries: %u) job reads=%u,%u jobs=%u,%u left to the host=%u,%u\n",
            c.n_reads, info[TI_RESOLVED], info[TI_WCUR], info[TI_WCUR + 1], info[TI_WWCUR], info[TI_WWCUR + 1], info[TI_W16WAVE], info[TI_CCUR],
            info[TI_CCUR + 1], info[TI_JCUR], info[TI_JCUR + 1], info[TI_JOVER], info[TI_JOVER + 1]);
    return WEPP_OK;
}

// stage 5.  The hints of the handle's next call, from this call's counters (they choose how a call cuts its work, never
// its results).  need_lists: a launch of this call reads the grouped read list.
void store_hints(const PlaceCall& c, bool need_lists) {
    wepp_mat_t* mat = c.mat;
    const uint32_t* info = c.L->h_info;
    if (c.f.walking) {
        // (see choose_form: scatter_blind)
        mat->expect_lists.store(need_lists ? ((c.f.lists_hint & 2u) ? 0u : 1u) : ((c.f.lists_hint & 1u) ? 2u : (c.f.lists_hint & 2u)), std::memory_order_relaxed);
        // the 8-entry job class is launched blind when this call held such reads
        mat->expect_jobs8.store(info[TI_CCUR] && !info[TI_JOVER] ? 1u : 0u, std::memory_order_relaxed);
    }
    for (uint32_t cc = 0; cc < 2; cc++) {
        const uint64_t ev = (uint64_t)info[TI_EVENTS + cc] << 6;
        const uint32_t je = (uint32_t)std::min<uint64_t>(WALK_JOB_EVENTS_MAX, std::max<uint64_t>(WALK_JOB_EVENTS, ev / WALK_TARGET_JOBS));
        mat->job_events[cc] = je <= WALK_JOB_EVENTS ? je : ((je + 15u) & ~15u);       // (what the NEXT call's k_route cuts this class's walks into)
    }
    // the reads with 17 - 256 events of the NEXT call: a wave per 64 events each while they are few (scaled to the call's size)
    const uint64_t scale = std::max<uint64_t>(1, ((uint64_t)c.n_reads + (1u << 20) - 1) >> 20);
    mat->ww_by_jobs.store((info[TI_WWCAND] > WW_CALL_MAX_SMALL * scale || info[TI_WWCAND + 1] > WW_CALL_MAX_BIG * scale) ? 1u : 0u, std::memory_order_relaxed);
    mat->step_walkers.store(info[TI_WCUR], std::memory_order_relaxed);      // (how the NEXT call's k_step places its plain walkers)
}

// stage 6.  What is launched from the counters.  k_scatter LATE: the hint said no and the counters say yes.  On ps, behind
// the copy and in front of everything that reads the lists (all of it is launched by the stages below, on ps or on
// streams forked from it).  Then the walk classes (joined into the caller's stream by join_and_account): the 8-entry job
// class when the hint did not expect it, and the classes of 9 - 16 entries, from k_route's tables like the others, when
// they hold reads.
int launch_late(PlaceCall& c, bool need_lists) {
    const uint32_t* info = c.L->h_info;
    const char* scatter_mode = "blind";
    if (c.f.walking && !c.scattered) {
        scatter_mode = need_lists ? "late" : "none";
        if (need_lists) HIP_TRY(scatter(c));
    }
    // Hazards of a call WITHOUT k_scatter (scattered == false from here on): nothing of this call reads blk_counts,
    // tier_of's slots or slot_in_blk -- per lane, rewritten by the lane's next k_route -- and nothing runs on ps -- by
    // report nothing was put there, by copy the host has seen the copy complete --, so ps needs no join.  k_step reads
    // this call's counter set (its two cursors; all of it for the report) on the caller's stream, in front of the next
    // k_route, which clears the OTHER set; the set after that clears this one, behind everything this call put on the caller's stream.  A k_scatter that was launched, blind or late,
    // reads those per-lane buffers and writes TI_OFF into this call's set: it and every consumer behind it are joined
    // into the caller's stream by join_and_account, before the call returns.
    if (c.mat->tun.debug_plans) fprintf(stderr, "[lists] scatter=%s plan stream joined=%d\n", scatter_mode, (int)(c.f.walking && c.scattered));
    if (!c.f.walking) return WEPP_OK;
    if (info[TI_CCUR] && !info[TI_JOVER] && !c.f.jobs8_blind) HIP_TRY(blind_side(c, PLAN_WALKC8, SIDE_JOBS8));
    if (info[TI_WCUR + 1]) HIP_TRY(blind_side(c, PLAN_WALK16, SIDE_WALK16));
    if (info[TI_CCUR + 1] && !info[TI_JOVER + 1]) HIP_TRY(blind_side(c, PLAN_WALKC16, SIDE_JOBS16));
    return WEPP_OK;
}

// ---- stage 8: the plans' launches.  What the chains share: the plan, the lists its tile plans read, the lane's
// second block, and which side streams hold a chain to join. ----
struct PlanLaunch : LaunchPlan {    // the plan, and what launching it adds
    char* part_base;
    size_t scan_temp[2], walkc_base[2];
    bool fork;
    uint32_t joins[MAX_STREAMS], n_joins;
};
struct Partials { int32_t* score; uint32_t *rank, *cnt; };
// the three partial arrays of n (chunk, read) pairs at part_off of the lane's second block
Partials parts(const PlanLaunch& pl, size_t part_off, size_t n) {
    int32_t* const score = (int32_t*)(pl.part_base + part_off);
    return Partials{score, (uint32_t*)(score + n), (uint32_t*)(score + n) + n};
}
const DevStream& stream_of(const wepp_mat_t* mat, const TilePlan& p) { return p.window ? mat->wstreams[p.sid] : mat->streams[p.sid]; }

// The lane's second block: the plans' partials and, behind them, what a chunked class the host plans itself
// needs -- jobs per read, their scan, the scan's scratch, three partials per job.  Nothing of this call has touched
// it; what the lane's previous call left running in it is waited for only when the block has to grow.
int reserve_partials(const PlaceCall& c, PlanLaunch& pl) {
    size_t part_need = pad256(pl.part_total);
    for (uint32_t cc = 0; cc < 2; cc++) {
        pl.scan_temp[cc] = pl.walkc_base[cc] = 0;
        if (!pl.walkc[cc].n) continue;
        HIP_TRY(scan_u32_temp_bytes(pl.walkc_reads[cc], &pl.scan_temp[cc]));
        pl.walkc_base[cc] = part_need;
        part_need += 2 * pad256((size_t)pl.walkc_reads[cc] * 4) + pad256(pl.scan_temp[cc]) + 3 * pad256((size_t)pl.n_jobs[cc] * 4);
    }
    // (half as much again: the partials of a batch of long reads vary by a third with the tile size its longest
    // read allows, and a regrowth costs a hipFree + hipMalloc of ~100 MB, 16 ms)
    WEPP_TRY(c.L->part.reserve(part_need, 2, "partials"));
    if (!c.scattered && (pl.np || pl.arena_n || pl.seed_n || pl.walkc[0].n || pl.walkc[1].n)) return set_error(WEPP_EDEVICE, "a planned launch without its read list");
    pl.part_base = (char*)c.L->part.ptr;
    pl.n_joins = 0;
    return WEPP_OK;
}

// the tile plans' lists; the reads that sweep the whole tree go by first listed position (sort_reads.hip); the fork
int sort_and_fork(const PlaceCall& c, PlanLaunch& pl) {
    const LaneRegions& r = c.r;
    for (uint32_t i = 0; i < pl.np; i++) {
        TilePlan& p = pl.plans[i];
        p.lst = r.list + p.off;
        if (c.mat->tun.debug_plans) print_plan_line(stderr, p);
        if (!p.window && p.t + 1 == c.mat->dev.n_streams && p.count >= SORT_MIN_READS) {
            HIP_TRY(launch_first_pos(r.list + p.off, p.count, c.rd.off, c.rd.word, r.key_in + p.off, c.f.ps));
            HIP_TRY(launch_sort_reads(r.key_in + p.off, r.key_out + p.off, r.list + p.off, r.val_in + p.off, p.count, r.sort_tmp, r.sort_temp, c.f.ps));
            p.lst = r.val_in + p.off;
        }
    }
    // Sweeps + finalizes: every chain beside the fused plain sweeps gets a side stream forked from / joined into ps --
    // behind the sorts -- when the call has more than one chain.  Every plan's finalize follows its sweep.
    const uint32_t n_walk_chains = (pl.walkc[0].n || pl.walkc[1].n) ? 1u : 0u;
    const uint32_t n_chains = pl.n_other + n_walk_chains + (pl.arena_n ? 1u : 0u) + (pl.seed_n ? 1u : 0u) + (pl.n_wins ? 1u : 0u);     // launch chains beside the fused plain sweeps
    pl.fork = (n_chains > 0) && (pl.n_plain > 0 || n_chains > 1);
    if (pl.fork) HIP_TRY(hipEventRecord(c.L->fork_ev, c.f.ps));
    return WEPP_OK;
}
// A chain beside the fused sweeps runs on side stream i (handle.hpp: SIDE_*) when the call forks, else on ps.
// The side streams join ps only after everything has been launched: a join in between would make the launches
// behind it wait for the side stream's kernels.  join(): the chain's last launch is queued; its stream is listed once.
hipError_t fork_to(const PlaceCall& c, const PlanLaunch& pl, uint32_t i, hipStream_t& q) {
    q = pl.fork ? c.L->side[i] : c.f.ps;
    return pl.fork ? hipStreamWaitEvent(q, c.L->fork_ev, 0) : hipSuccess;
}
hipError_t join(const PlaceCall& c, PlanLaunch& pl, uint32_t i) {
    if (!pl.fork) return hipSuccess;
    const hipError_t e = hipEventRecord(c.L->join_ev[i], c.L->side[i]);
    if (e == hipSuccess && std::find(pl.joins, pl.joins + pl.n_joins, i) == pl.joins + pl.n_joins) pl.joins[pl.n_joins++] = i;
    return e;
}

// A walk class's reads go by (stream, first listed position) when there are enough of them (device_mat.hpp:
// WALK_SORT_MIN_READS): sorted on the class's own stream, right before its launch.
// `region` = which of the sort temp regions (1..4; 0 is the whole-tree plan's).  lst: the class's list, sorted or not.
int sort_class(const PlaceCall& c, uint32_t cls, uint32_t region, hipStream_t q, const uint32_t*& lst) {
    const LaneRegions& r = c.r;
    const uint32_t off = c.L->h_info[TI_OFF + plan_id(cls, 0)];
    const uint32_t cnt = c.L->h_info[TI_OFF + plan_id(cls, 0) + MAX_STREAMS] - off;      // (plan ids of a class are consecutive)
    lst = r.list + off;
    if (cnt < WALK_SORT_MIN_READS) return WEPP_OK;
    HIP_TRY(launch_walk_keys(r.list + off, cnt, c.tier_of, c.rd.off, c.rd.word, r.key_in + off, q));
    HIP_TRY(launch_sort_reads(r.key_in + off, r.key_out + off, r.list + off, r.val_in + off, cnt, (char*)r.sort_tmp + region * r.sort_temp,
                              r.sort_temp, q, WALK_SORT_KEY_BITS));
    lst = r.val_in + off;
    return WEPP_OK;
}

// The chunked walks the host plans itself.  The walks write the final per-read results themselves; the plain ones, the
// chunked ones and the sweeps run side by side (the walks wait on memory most of the time).  Per class: jobs per read
// in list order -> exclusive scan -> the walk (a partial per job; a job finds its read by bisection in the scanned
// offsets) -> one combination per read.  Buffers: each class's share of the lane's second block, behind the plans'
// partials (reserve_partials).
int launch_chunked_walks(const PlaceCall& c, PlanLaunch& pl) {
    for (uint32_t cc = 0; cc < 2; cc++) {
        if (!pl.walkc[cc].n) continue;
        // each class on a side stream of its own: a chain of short, latency-bound launches
        const uint32_t side = cc ? SIDE_JOBS16 : SIDE_JOBS8;
        hipStream_t q;
        HIP_TRY(fork_to(c, pl, side, q));
        const uint32_t R3 = pl.walkc_reads[cc], J = (uint32_t)pl.n_jobs[cc];
        const size_t b_cnt = pad256((size_t)R3 * 4), b_tmp = pad256(pl.scan_temp[cc]), b_job = pad256((size_t)J * 4);
        char* w2 = pl.part_base + pl.walkc_base[cc];
        uint32_t* jcnt = (uint32_t*)w2; w2 += b_cnt;
        uint32_t* joff = (uint32_t*)w2; w2 += b_cnt;
        void* jtmp = w2; w2 += b_tmp;
        WalkJobs jb{};
        jb.n_list = R3;
        jb.job_off = joff;
        jb.job_n = c.r.job_n;
        jb.part_score = (int32_t*)w2; w2 += b_job;
        jb.part_rank = (uint32_t*)w2; w2 += b_job;
        jb.part_cnt = (uint32_t*)w2;
        const uint32_t* list3 = nullptr;
        WEPP_TRY(sort_class(c, PLAN_WALKC8 + cc, 3 + cc, q, list3));
        WalkPlans wp = pl.walkc[cc];
        for (uint32_t k = 0; k < wp.n; k++) wp.p[k].list = list3;
        HIP_TRY(launch_gather_jobs(list3, R3, c.r.job_n, jcnt, q));
        HIP_TRY(launch_exclusive_scan_u32(jcnt, joff, R3, jtmp, pl.scan_temp[cc], q));
        HIP_TRY(launch_walk_jobs(c.mat->dev, wp, PLAN_WALKC8 + cc, c.L->h_info[TI_OPEN + 2 + cc], jb, c.rd, c.mat->d_work, q));
        HIP_TRY(launch_finalize_jobs(c.mat->dev, list3, R3, jb, c.out, q));
        HIP_TRY(join(c, pl, side));
    }
    return WEPP_OK;
}

// the dense and out-of-LDS plans: a launch each, on the side streams in turn
int launch_own_plans(const PlaceCall& c, PlanLaunch& pl) {
    for (uint32_t k = 0; k < pl.n_other; k++) {
        const uint32_t i = pl.others[k];
        const TilePlan& p = pl.plans[i];
        hipStream_t q;
        HIP_TRY(fork_to(c, pl, k % OTHER_SIDE_STREAMS, q));
        const Partials pt = parts(pl, p.part_off, (size_t)p.nchunks * p.count);
        HIP_TRY(launch_sweep(c.mat->dev, stream_of(c.mat, p), c.rd, p.lst, p.count, p.T, p.ntiles, p.nchunks, p.bpc, p.s_in_lds, p.dense, p.win_table, p.ent_cap,
                             p.key_cap, p.lds_bytes, pt.score, pt.rank, pt.cnt, q));
        HIP_TRY(launch_finalize(c.mat->dev, c.rd, p.lst, p.count, p.nchunks, pt.score, pt.rank, pt.cnt, c.out, q));
        if (k + OTHER_SIDE_STREAMS >= pl.n_other) HIP_TRY(join(c, pl, k % OTHER_SIDE_STREAMS));     // (the last of these launches on its side stream)
    }
    return WEPP_OK;
}

// what the records of the two fused launches (SweepPlanDev, WinPlanDev) share; wg_per_tile: sweep workgroups of a tile
template <typename Dev>
void fill_fused(Dev& d, const PlanLaunch& pl, const TilePlan& p, uint32_t wg_per_tile, uint32_t& wg, uint32_t& fin, uint32_t& lds_max) {
    const Partials pt = parts(pl, p.part_off, (size_t)p.nchunks * p.count);
    d.list = p.lst;
    d.n_list = p.count; d.T = p.T; d.ntiles = p.ntiles; d.bpc = p.bpc; d.ent_cap = p.ent_cap; d.nchunks = p.nchunks;
    d.part_score = pt.score; d.part_rank = pt.rank; d.part_cnt = pt.cnt;
    d.wg_end = wg += p.ntiles * wg_per_tile;
    d.fin_end = fin += finalize_blocks(p.count, p.nchunks);
    lds_max = std::max(lds_max, p.lds_bytes);
}

// the table window plans, fused into one launch
int launch_window_plans(const PlaceCall& c, PlanLaunch& pl) {
    if (!pl.n_wins) return WEPP_OK;
    WinPlans wp{};
    uint32_t wg = 0, fin = 0, lds_max = 0;
    for (uint32_t k = 0; k < pl.n_wins; k++) {
        const TilePlan& p = pl.plans[pl.wins[k]];
        wp.p[k].sid = p.sid;
        wp.p[k].win_base = p.key_cap;
        fill_fused(wp.p[k], pl, p, p.nchunks / DENSE_WAVES_PER_WG, wg, fin, lds_max);
    }
    wp.n = pl.n_wins;
    hipStream_t q;
    HIP_TRY(fork_to(c, pl, SIDE_WINDOWS, q));
    HIP_TRY(launch_sweep_windows(c.mat->dev, c.mat->d_wstreams, wp, c.rd, lds_max, q));
    HIP_TRY(launch_finalize_windows(c.mat->dev, wp, c.rd, c.out, q));
    HIP_TRY(join(c, pl, SIDE_WINDOWS));
    return WEPP_OK;
}

// the reads that sweep their window crown (k_sweep_arena)
int launch_arena(const PlaceCall& c, PlanLaunch& pl) {
    if (!pl.arena_n) return WEPP_OK;
    const uint32_t cap = (pl.arena_maxk + 63) & ~63u;
    const uint32_t* lst = c.r.list + pl.arena_off;
    hipStream_t q;
    HIP_TRY(fork_to(c, pl, SIDE_ARENA, q));
    const Partials pt = parts(pl, pl.arena_part, (size_t)pl.arena_n * ARENA_CHUNKS);
    HIP_TRY(launch_sweep_arena(c.mat->dev, c.mat->dev.wc_streams, c.rd, lst, pl.arena_n, cap, sweep_lds_bytes(c.mat->dev.bm_words, cap, 0, false), pt.score, pt.rank, pt.cnt, q));
    HIP_TRY(launch_finalize(c.mat->dev, c.rd, lst, pl.arena_n, ARENA_CHUNKS, pt.score, pt.rank, pt.cnt, c.out, q));
    HIP_TRY(join(c, pl, SIDE_ARENA));
    return WEPP_OK;
}

// the seeded samples (k_seed)
int launch_seeds(const PlaceCall& c, PlanLaunch& pl) {
    const wepp_mat_t* mat = c.mat;
    if (!pl.seed_n) return WEPP_OK;
    if (pl.seed_maxk > SEED_MAX_ENTRIES) return set_error(WEPP_EDEVICE, "routing seeded a sample with too many entries");
    const uint32_t cap = (pl.seed_maxk + 63) & ~63u;
    hipStream_t q;
    HIP_TRY(fork_to(c, pl, SIDE_SEED, q));
    if (mat->tun.debug_plans) fprintf(stderr, "[plan] seed count=%u maxk=%u chunks=%u lds=%u\n", pl.seed_n, pl.seed_maxk, mat->dev.seed_chunks, seed_lds_bytes(mat->dev, cap));
    HIP_TRY(launch_seed(mat->dev, mat->streams.back(), c.r.list + pl.seed_off, pl.seed_n, cap, c.rd, c.out, mat->d_work, mat->tun.seed_heavy ? c.L->d_seed_heavy.ptr : nullptr, q));
    HIP_TRY(join(c, pl, SIDE_SEED));
    return WEPP_OK;
}

// the plain (short-read) plans, fused into one launch on the plan stream
int launch_plain_plans(const PlaceCall& c, const PlanLaunch& pl) {
    if (!pl.n_plain) return WEPP_OK;
    SweepPlans sp{};
    uint32_t wg = 0, fin = 0, lds_max = 0;
    for (uint32_t k = 0; k < pl.n_plain; k++) {
        const TilePlan& p = pl.plans[pl.order[k]];
        sp.p[k].st = stream_of(c.mat, p);
        fill_fused(sp.p[k], pl, p, p.nchunks, wg, fin, lds_max);
    }
    sp.n = pl.n_plain;
    HIP_TRY(launch_sweep_multi(c.mat->dev, sp, c.rd, lds_max, c.f.ps));
    HIP_TRY(launch_finalize_multi(c.mat->dev, sp, c.rd, c.out, c.f.ps));
    return WEPP_OK;
}

// stage 9.  The side streams' chains join the plan stream, the plan stream and the walks' side streams the caller's;
// the call's second time stamp and its statistics.
int join_and_account(const PlaceCall& c, const PlanLaunch& pl, uint32_t plan_total) {
    wepp_mat_t* mat = c.mat;
    PlaceLane& L = *c.L;
    const CallForm& f = c.f;
    for (uint32_t i = 0; i < pl.n_joins; i++) HIP_TRY(hipStreamWaitEvent(f.ps, L.join_ev[pl.joins[i]], 0));
    bool joined = false;              // something was joined into the caller's stream behind k_step
    if (f.walking) {
        // the plan stream, when something ran on it behind the counters' copy (k_scatter and what reads its lists: no
        // consumer is launched without it), and the blind walks' side streams join the caller's stream
        if (c.scattered) {
            HIP_TRY(hipEventRecord(L.join_ev[SIDE_PLAN], f.ps));
            HIP_TRY(hipStreamWaitEvent(c.stream, L.join_ev[SIDE_PLAN], 0));
        }
        for (uint32_t i : {SIDE_WAVE, SIDE_JOBS8, SIDE_WALK16, SIDE_JOBS16})
            if (c.walk_sides >> i & 1u) HIP_TRY(hipStreamWaitEvent(c.stream, L.join_ev[i], 0));
        joined = c.scattered || c.walk_sides;
    }
    // (the end of the timed span: k_step's own stop event when the kernel is the call's last work on the caller's
    // stream, else a record behind the joins -- which takes the event over from the launch)
    if (!c.ev1_on_step || joined) HIP_TRY(hipEventRecord(mat->ev1[f.ev_slot], c.stream));
    std::lock_guard<std::mutex> lk(mat->stat_mu);
    mat->last_passes = pl.passes;
    mat->last_bytes = pl.bytes;
    mat->acc_passes += pl.passes;
    mat->acc_bytes += pl.bytes;
    if (plan_total == c.n_reads) {            // a call of its own
        mat->last_n_reads = c.n_reads;
        mat->last_walk_reads = pl.walk_reads;
    } else {                                // a sub-batch (wepp_place_batch reset the sums): complete once every one is in, in any order
        mat->plan_reads_in += c.n_reads;
        mat->last_walk_reads += pl.walk_reads;
        mat->last_n_reads = mat->plan_reads_in == plan_total ? plan_total : 0;
    }
    return WEPP_OK;
}

}  // namespace

// Two sub-batches of one wepp_place_batch may be inside this function at once, on two host threads and two lanes, and
// even with one host thread their kernels may overlap on the device (each lane has its own compute stream).  Each lane
// has its own two device blocks (handle.hpp: the fixed regions, grown before k_route, and the partials, grown once the
// routing counters are back: a call routes once, whatever its partials need), routing counters, side streams, events
// and k_seed second-pass table.  What they share on the handle:
//   - the tree and everything built from it (read-only here);
//   - the event ring (a slot claimed atomically: choose_form);
//   - the hints job_events, ww_by_jobs, step_walkers, expect_jobs8 and expect_lists (atomics, read by choose_form and written by store_hints; they choose how the next call cuts its work, never its results);
//   - the call statistics (stat_mu: join_and_account) and the device counters d_work (device atomics, summed over both lanes);
//   - d_plan_of / d_wsid_of, of which each sub-batch writes only its own range [plan_base, plan_base + n_reads).
int place_device(wepp_mat_t* mat, const uint32_t* d_read_off, const uint32_t* d_read_word, uint32_t n_reads,
                 uint32_t* d_best_bfs_j, int32_t* d_score, uint32_t* d_num_best, uint32_t* d_flags, hipStream_t stream,
                 uint32_t plan_base, uint32_t plan_total, uint32_t lane_idx) {
    // (a pipelined wepp_place_batch has sized them for the whole call before its sub-batches start, on one thread)
    WEPP_TRY(ensure_plan_buffers(mat, plan_total));
    PlaceCall c{mat, &mat->lane[lane_idx], CallReads{d_read_off, d_read_word, nullptr, nullptr}, CallResults{d_best_bfs_j, d_score, d_num_best, d_flags}, n_reads, stream};
    WEPP_TRY(carve_workspace(c, plan_base));
    c.f = choose_form(mat, *c.L, n_reads, stream);
    WEPP_TRY(route_and_launch_blind(c));
    WEPP_TRY(wait_counters(c));
    // Who reads `list`: decided HERE, from the counters, for the whole call.
    const bool need_lists = !c.f.walking || lists_needed(c.L->h_info);
    store_hints(c, need_lists);
    WEPP_TRY(launch_late(c, need_lists));
    PlanLaunch pl;
    WEPP_TRY(plan_launches(c.L->h_info, mat->tile_reads, c.f.walking, mat->d_wstreams != nullptr, mat->dev, mat->streams.data(), mat->stream_bytes.data(),
                           mat->wstreams.data(), mat->wstream_bytes.data(), (uint32_t)mat->wstreams.size(), pl));
    WEPP_TRY(reserve_partials(c, pl));
    WEPP_TRY(sort_and_fork(c, pl));
    // (the chains in the order the side streams have always got them)
    WEPP_TRY(launch_chunked_walks(c, pl));
    WEPP_TRY(launch_own_plans(c, pl));
    WEPP_TRY(launch_window_plans(c, pl));
    WEPP_TRY(launch_arena(c, pl));
    WEPP_TRY(launch_seeds(c, pl));
    WEPP_TRY(launch_plain_plans(c, pl));
    return join_and_account(c, pl, plan_total);
}
}  // namespace wepp

extern "C" int wepp_place_batch_device(wepp_mat_t* mat, const uint32_t* d_read_off, const uint32_t* d_read_word,
                                       uint32_t n_reads, uint64_t n_read_words, uint32_t* d_best_bfs_j,
                                       int32_t* d_score, uint32_t* d_num_best, uint32_t* d_flags,
                                       void* hip_stream) {
    if (!mat || !d_read_off) return set_error(WEPP_EINVAL, "null argument");
    if (n_read_words && !d_read_word) return set_error(WEPP_EINVAL, "null read_word");
    if (n_reads == 0) return WEPP_OK;
    HIP_TRY(hipSetDevice(mat->device));
    return place_device(mat, d_read_off, d_read_word, n_reads, d_best_bfs_j, d_score, d_num_best, d_flags,
                        (hipStream_t)hip_stream, 0, n_reads);
}

namespace {
// `n` slots of the handle's device counters from slot `first` on (handle.hpp: d_work)
int read_work_slots(wepp_mat_t* mat, uint32_t first, uint32_t n, unsigned long long* out) {
    HIP_TRY(hipMemcpy(out, mat->d_work + first, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return WEPP_OK;
}

// the plan id of every read of the handle's most recent placement call, for the diagnostics that decode it
int read_last_plans(wepp_mat_t* mat, uint8_t* plan_ids, uint32_t n_reads) {
    if (n_reads != mat->last_n_reads || !mat->d_plan_of)
        return set_error(WEPP_EINVAL, "n_reads differs from the handle's last placement call");
    HIP_TRY(hipSetDevice(mat->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(plan_ids, mat->d_plan_of, n_reads, hipMemcpyDeviceToHost));
    return WEPP_OK;
}
}  // namespace

extern "C" int wepp_mat_timing_reset(wepp_mat_t* mat) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    mat->n_timed = 0;
    mat->acc_passes = mat->acc_bytes = 0;
    HIP_TRY(hipSetDevice(mat->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(mat->d_work, 0, wepp_mat::D_WORK_BYTES));
    return WEPP_OK;
}

extern "C" int wepp_mat_last_timing(wepp_mat_t* mat, float* mean_sweep_ms, uint32_t* n_calls, uint64_t* passes,
                                    uint64_t* algorithmic_bytes) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    if (mat->n_timed == 0) return set_error(WEPP_EINVAL, "no placement has been launched on this handle since the last reset");
    HIP_TRY(hipSetDevice(mat->device));
    const uint32_t n = (uint32_t)std::min<uint64_t>(mat->n_timed, wepp_mat::kRing);
    double sum = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t slot = (uint32_t)((mat->n_timed - 1 - i) % wepp_mat::kRing);
        HIP_TRY(hipEventSynchronize(mat->ev1[slot]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, mat->ev0[slot], mat->ev1[slot]));
        sum += ms;
    }
    // what the walks asked memory for: counted by their lanes (k_walk: a 32-byte index entry per node event, the
    // sparse-table bytes and range-query aggregates actually requested, list heads, read words, start states of
    // the jobs, results); averaged over the calls since the reset
    unsigned long long wb = 0;
    std::vector<unsigned long long> slots(WALK_COUNTERS);
    WEPP_TRY(read_work_slots(mat, WALK_COUNTERS, WALK_COUNTERS, slots.data()));
    for (unsigned long long v : slots) wb += v;
    if (mean_sweep_ms) *mean_sweep_ms = (float)(sum / n);
    if (n_calls) *n_calls = n;
    if (passes) *passes = mat->acc_passes / std::max<uint64_t>(1, mat->n_timed);
    if (algorithmic_bytes) *algorithmic_bytes = (mat->acc_bytes + wb) / std::max<uint64_t>(1, mat->n_timed);
    return WEPP_OK;
}

// diagnostic: the sweep stream every read of the handle's most recent placement call was routed to
extern "C" int wepp_mat_last_tiers(wepp_mat_t* mat, uint8_t* tiers, uint32_t n_reads) {
    if (!mat || !tiers) return set_error(WEPP_EINVAL, "null argument");
    WEPP_TRY(read_last_plans(mat, tiers, n_reads));
    for (uint32_t r = 0; r < n_reads; r++)       // the workspace holds plan ids (device_mat.hpp: plan_id)
        tiers[r] = (plan_class(tiers[r]) == PLAN_WIN || plan_class(tiers[r]) == PLAN_SEED) ? (uint8_t)(mat->dev.n_streams - 1) : (uint8_t)plan_index(tiers[r]);
    return WEPP_OK;
}

// diagnostic: the full plan id (class and stream) of every read of the handle's most recent placement call
extern "C" int wepp_mat_last_plans(wepp_mat_t* mat, uint8_t* plan_class_out, uint8_t* plan_stream_out, uint32_t n_reads) {
    if (!mat || !plan_class_out || !plan_stream_out) return set_error(WEPP_EINVAL, "null argument");
    WEPP_TRY(read_last_plans(mat, plan_stream_out, n_reads));
    for (uint32_t r = 0; r < n_reads; r++) {
        const uint32_t id = plan_stream_out[r];
        plan_class_out[r] = (uint8_t)plan_class(id);
        plan_stream_out[r] = (uint8_t)plan_index(id);
    }
    return WEPP_OK;
}

// diagnostic: the window crown (window, crown of the window) of every read of the last call that walked one
extern "C" int wepp_mat_last_crowns(wepp_mat_t* mat, uint8_t* window_out, uint8_t* crown_out, uint32_t n_reads) {
    if (!mat || !window_out || !crown_out) return set_error(WEPP_EINVAL, "null argument");
    std::vector<uint32_t> sid(n_reads);
    std::vector<uint8_t> plan(n_reads);
    WEPP_TRY(read_last_plans(mat, plan.data(), n_reads));
    HIP_TRY(hipMemcpy(sid.data(), mat->d_wsid_of, (size_t)n_reads * 4, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < n_reads; r++) {
        const bool in_arena = plan_class(plan[r]) != PLAN_WIN && plan_class(plan[r]) != PLAN_SWEEP && plan_index(plan[r]) == WC_SLOT;
        window_out[r] = in_arena ? (uint8_t)(sid[r] / WC_MAX) : (uint8_t)255;
        crown_out[r] = in_arena ? (uint8_t)(sid[r] % WC_MAX) : (uint8_t)255;
    }
    return WEPP_OK;
}

// diagnostic: how the most recent placement call placed its reads
extern "C" int wepp_mat_last_walk(wepp_mat_t* mat, uint64_t* reads_walked, uint64_t* walk_iterations) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(mat->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long it = 0;
    std::vector<unsigned long long> slots(WALK_COUNTERS);
    WEPP_TRY(read_work_slots(mat, 0, WALK_COUNTERS, slots.data()));
    for (unsigned long long v : slots) it += v;
    if (reads_walked) *reads_walked = mat->last_walk_reads;
    if (walk_iterations) *walk_iterations = it;
    if (mat->tun.walk_debug) {
        unsigned long long a = 0, b = 0;
        for (uint32_t i = 0; i < WALK_COUNTERS / 2; i++) { a += slots[i]; b += slots[WALK_COUNTERS / 2 + i]; }
        fprintf(stderr, "[walk] wave-iterations since reset: plain %llu chunked %llu\n", a, b);
        // -DWEPP_WALK_STATS builds: slots 0..6 / 16..22 = wave cycles by phase (decode, stage, start state, walk, write), waves, iterations
        for (int c = 0; c < 2; c++) {
            const unsigned long long* v = slots.data() + c * 16;
            if (v[5] && v[5] < (1ull << 40))
                fprintf(stderr, "[walk stats] %s: waves %llu iterations/wave %.1f cycles/wave: decode %.0f stage %.0f start-state %.0f walk %.0f write %.0f\n",
                        c ? "chunked" : "plain", v[5], (double)v[6] / v[5], (double)v[0] / v[5], (double)v[1] / v[5], (double)v[2] / v[5],
                        (double)v[3] / v[5], (double)v[4] / v[5]);
            if (v[5] && v[5] < (1ull << 40))
                fprintf(stderr, "[walk stats] %s: lanes with work %llu  lane-iterations %llu (%.1f per lane, %.1f%% of wave-iterations x 64)  node events %llu  "
                        "table bytes %llu  exact range queries %llu\n", c ? "chunked" : "plain", v[11], v[7], (double)v[7] / std::max(1ull, v[11]),
                        100.0 * v[7] / std::max(1.0, 64.0 * v[6]), v[8], v[9], v[10]);
        }
    }
    return WEPP_OK;
}

// diagnostic: the whole-genome samples the handle seeded since the last timing reset, the chunks of the whole-tree
// stream they evaluated and the chunks they could have evaluated (samples x chunks of the tree)
extern "C" int wepp_mat_last_seeds(wepp_mat_t* mat, uint64_t* samples, uint64_t* chunks_evaluated, uint64_t* chunks_total,
                                   uint64_t* most_per_sample, uint64_t* histogram8) {
    if (!mat) return set_error(WEPP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(mat->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v[12] = {};
    WEPP_TRY(read_work_slots(mat, 2 * WALK_COUNTERS, 12, v));
    if (samples) *samples = v[0];
    if (chunks_evaluated) *chunks_evaluated = v[1];
    if (chunks_total) *chunks_total = v[2];
    if (most_per_sample) *most_per_sample = v[3];
    if (histogram8)
        for (int i = 0; i < 8; i++) histogram8[i] = v[4 + i];
    return WEPP_OK;
}
