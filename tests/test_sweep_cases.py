"""tests/sweep_cases.py held to its edges on the CPU: the restated launch rule at its thresholds, and for every builder
the fact about its INPUT that makes it an edge case -- entry counts on both sides of a threshold, hit events per block
of the flat image, positions against the tile's smallest one, chunk lengths, oracle answers that change with the word
a confused kernel would misread.  A generator that drifts cannot hollow a case out unnoticed.  Every case on a small
tree also goes through the Python model of the sweep (tests/sweep_model.py), cut into the chunks the rule predicts,
against the oracle.  The library's own planner (wepp_amd/csrc/launch_plan.hpp) is held to the same rule without a GPU:
tests/cxx/launch_plan_main.cpp plans every tile case and prints the `[plan]` lines the device call would."""
import os
import subprocess

import numpy as np
import pytest

import sweep_cases as sc
import sweep_model as sm
from wepp_amd import Reads


# ---- the rule ----------------------------------------------------------------------------------------------------------
def test_tile_rule_thresholds():
    assert [sc.tile_reads(k) for k in (1, 128, 129, 256, 257, 4096, 4097, 8192, 8193, 100000)] == [64, 64, 32, 32, 16, 2, 1, 1, 1, 1]
    assert [sc.tile_reads(k, 16) for k in (1, 512, 513)] == [16, 16, 8] and sc.tile_reads(5, 1) == 1
    assert not sc.takes_table(15, 2000) and sc.takes_table(16, 2000) and sc.takes_table(8192, 2000) and not sc.takes_table(8193, 2000)
    # position field 2^19 - 1 of a key is reserved: the tree's positions stay below it
    assert sc.takes_table(16, (1 << 19) - 2) and not sc.takes_table(16, (1 << 19) - 1) and not sc.takes_table(16, 1 << 19)
    assert sc.ent_cap(5, 1) == 64 and sc.ent_cap(5, 64) == 320 and sc.ent_cap(5, 65) == 320 and sc.ent_cap(65, 1) == 128
    assert sc.ent_cap(128, 64) == 8192 and sc.ent_cap(129, 64) == 4160 and sc.ent_cap(8192, 3) == 8192 and sc.ent_cap(8193, 3) == 0
    assert sc.key_cap(16, 1, 2000) == 64 and sc.key_cap(16, 64, 2000) == 1024 and sc.key_cap(17, 64, 2000) == 2048
    assert sc.key_cap(129, 64, 2000) == 8192 and sc.key_cap(15, 64, 2000) == 0 and sc.key_cap(16, 64, 1 << 19) == 0


def test_chunk_rule():
    # few tiles on a small stream: chunks of NB / 8 blocks' worth of checkpoints
    assert sc.chunks(1, 71, 71, 1, 30000, False, 3) == (8, 9) and sc.chunks(1, 72, 72, 1, 30000, False, 3) == (9, 8)
    assert sc.chunks(1, 256, 256, 1, 120000, False, 3) == (32, 8) and sc.chunks(1, 264, 264, 1, 120000, False, 3) == (33, 8)
    assert sc.chunks(1, 1024, 1024, 1, 480000, False, 3) == (128, 8) and sc.chunks(1, 1032, 516, 2, 480000, False, 3) == (129, 8)
    # 4096 tiles and more: one chunk per tile
    assert sc.chunks(4095, 60, 60, 1, 30000, False, 4095) == (2, 30) and sc.chunks(4096, 60, 60, 1, 30000, False, 4096) == (1, 60)
    # dense: a chunk per wave of the workgroup, rounded up to whole workgroups (the last ones may be empty)
    assert sc.chunks(1, 32, 32, 1, 15000, True, 3) == (16, 2) and sc.chunks(1, 36, 36, 1, 15000, True, 3) == (16, 3)
    assert sc.chunks(1, 7, 7, 1, 3000, True, 3) == (16, 1) and sc.chunks(1, 100, 100, 1, 50000, True, 3) == (16, 7)
    # a stream of several MB: a chunk per MB; the table window plans of a call share their target
    assert sc.chunks(4096, 60000, 1024, 59, 40 << 20, False, 4096) == (40, 1534)
    assert sc.chunks(2, 26, 26, 1, 9000, True, 70, win_tiles=2) == (16, 2)
    assert [sc.finalize_lanes_per_read(n) for n in (1, 8, 9, 32, 33, 128, 129, 4096)] == [1, 1, 4, 4, 16, 16, 64, 64]
    assert [sc.finalize_reads_per_workgroup(n) for n in (8, 9, 33, 129)] == [256, 64, 16, 4]


def test_plan_line_parser():
    d = sc.parse_plan_line("[plan] window t=6 count=70 off=0 T=64 ntiles=2 nchunks=16 bpc=2 NB=32 ncp=32 dense=1 lds=123 ent_cap=1024 key_cap=1024 part_off=0")
    assert d["kind"] == "window" and d["T"] == 64 and d["key_cap"] == 1024 and d["part_off"] == 0


def test_tiles_keep_the_batch_order_and_sort_from_4096_reads():
    lists = [[(50 - i % 50, 1, 2, 0)] for i in range(100)]
    assert sc.tiles_of(lists)[0] == list(range(64)) and sc.tiles_of(lists)[1] == list(range(64, 100))
    big = [[(1 + (i * 7) % 100, 1, 2, 0)] if i % 9 else [] for i in range(4096)]
    tiles = sc.tiles_of(big, 1)
    firsts = [big[t[0]][0][0] + 1 if big[t[0]] else 0 for t in tiles]
    assert firsts == sorted(firsts) and firsts[0] == 0 and tiles[0] == [0] and len(tiles) == 4096


# ---- the builders --------------------------------------------------------------------------------------------------------
def _k(case):
    return np.diff(case.reads.read_off.astype(np.int64))


def test_tile_rule_cases():
    c15, c16 = sc.CASES["maxk_15"](), sc.CASES["maxk_16"]()
    assert c15.reads.n_reads == c16.reads.n_reads == 70 and _k(c15).max() == 15 and _k(c16).max() == 16
    assert (c15.plan()["dense"], c16.plan()["dense"]) == (0, 1) and c15.plan()["ntiles"] == 2
    assert [len(t) for t in sc.tiles_of(c16.lists())] == [64, 6]
    c128, c129 = sc.CASES["maxk_128"](), sc.CASES["maxk_129"]()
    assert (_k(c128) == 128).all() and c128.reads.n_reads == 64 and c128.facts["n_ent"] == [(8192, 8192)]
    assert sorted(_k(c129).tolist()) == [128] * 63 + [129] and (c128.plan()["T"], c129.plan()["T"]) == (64, 32)
    assert c129.facts["n_ent"] == [(4096, 4096), (4097, 8192)]
    a, b = sc.CASES["maxk_8192"](), sc.CASES["maxk_8193"]()
    assert _k(a).tolist() == [20, 8192, 7] and _k(b).tolist() == [20, 8193, 7]
    pa, pb = a.plan(), b.plan()
    assert (pa["T"], pa["dense"], pa["ent_cap"], pa["key_cap"]) == (1, 1, 8192, 8192) and a.facts["n_ent"][1] == (8192, 8192)
    assert (pb["T"], pb["dense"], pb["ent_cap"], pb["key_cap"]) == (1, 0, 0, 0)
    for n in (1, 64, 65):
        for kind, k, dense in (("plain", 5, 0), ("dense", 18, 1)):
            c = sc.CASES["count_%d_%s" % (n, kind)]()
            assert c.reads.n_reads == n and (_k(c) == k).all() and c.plan()["dense"] == dense
            assert [len(t) for t in sc.tiles_of(c.lists())] == ([64, 1] if n == 65 else [n])
    for t in (1, 16, 64):
        for kind, dense in (("plain", 0), ("dense", 1)):
            c = sc.CASES["tile_%d_%s" % (t, kind)]()
            p = c.plan()
            assert c.knobs["tile"] == t and (p["T"], p["ntiles"], p["dense"]) == (t, -(-70 // t), dense)


def _answers(ot, lists):
    got = ot.place_batch(Reads.from_lists(lists), 4)
    return [tuple(int(got[f][i]) for f in ("score", "best_j", "num_best", "has_unique")) for i in range(len(lists))]


def test_plain_variant_cases(oracle):
    one, sep, same = (sc.CASES[n]() for n in ("own_4_and_5_one_tile", "own_4_and_5_separate_tiles", "own_identical_reads"))
    assert one.facts["tiles"] == [[4, 5] * 27]
    assert [sorted(set(t)) for t in sep.facts["tiles"]] == [[4], [4, 5], [5], [5]]
    ot = oracle.OracleTree(one.tree)
    # the fifth word -- the only one the plain sweep does not keep in a register -- decides the placement
    lists = one.lists()
    five = [l for l in lists if len(l) == 5]
    assert len(five) == 27 and all(l[4][0] == max(e[0] for e in l) for l in five)
    full, cut = _answers(ot, five), _answers(ot, [l[:4] for l in five])
    assert sum(a != b for a, b in zip(full, cut)) >= 20 and all(a[0] == 0 for a in full)
    assert [l[:4] for l in five] == [l for l in lists if len(l) == 4]
    # identical reads side by side in one tile, and in different tiles
    k = same.facts["k"]
    for a, b, one_tile, equal in same.facts["pairs"]:
        assert equal and k[a] == k[b]
    assert [(k[a], t) for a, b, t, _ in same.facts["pairs"]] == [(4, True), (5, True), (4, False), (5, False), (4, False), (5, False), (4, False)]
    assert same.reads.n_reads == 130 and same.plan()["ntiles"] == 3


def test_dense_key_cases():
    run = sc.CASES["dense_run_of_64"]()
    f = run.facts
    assert run.reads.n_reads == 64 and f["listing_q"] == 64 and f["hits_in_block"] >= sc.DENSE_MIN_HITS and run.plan()["dense"] == 1
    assert f["block"] in run.info.blocks_of(f["q"])
    win = sc.CASES["dense_window"]()
    f = win.facts
    assert f["at_4095"] == f["plo"] + sc.DENSE_WINDOW - 1 and f["at_4096"] == f["plo"] + sc.DENSE_WINDOW and f["far"] > f["plo"] + 4 * sc.DENSE_WINDOW
    assert all(f["listed"][x] == 8 for x in f["listed"]) and all(h >= sc.DENSE_MIN_HITS for h in f["hits"].values())
    assert all(win.info.blocks_of(x) for x in (f["at_4095"], f["at_4096"], f["far"])) and win.plan()["dense"] == 1
    a, b = sc.CASES["dense_n_ent_1024"](), sc.CASES["dense_n_ent_1025"]()
    assert a.facts["n_ent"] == [(1024, 1024)] and b.facts["n_ent"] == [(1025, 2048)] and _k(a).min() == 16
    h = sc.CASES["dense_hits_2_and_3"]()
    assert (h.facts["hits_b2"], h.facts["hits_b3"], h.facts["hit_blocks"]) == (2, 3, 2) and h.facts["b2"] != h.facts["b3"]
    assert h.plan()["dense"] == 1 and (_k(h) == 16).all()
    assert sc.hit_facts(h.info, h.lists()) == [dict(few=1, many=1, over128=0)]


def test_position_cases(oracle):
    H = 1 << 19
    for kind, k, dense in (("plain", 5, 0), ("dense", 18, 1)):
        for tag in "ab":
            c = sc.CASES["pos_%s_%s" % (tag, kind)]()
            f, lists = c.facts, c.lists()
            q = f["q"]
            assert (_k(c) == k).all() and c.plan()["dense"] == dense and f["block"] in c.info.blocks_of(q)
            if dense:
                assert f["hits_in_block"] >= sc.DENSE_MIN_HITS       # q's event is looked up by its lane
                # the read is placed on D, a descendant of the node X that mutates q, one block further in the same
                # chunk: what X's enter event adds to the read's running count decides D's score
                n0, d2i = c.info.flat.get("blk_node0"), c.info.flat.get("dfs2id").tolist()
                blk = lambda node: int(np.searchsorted(n0, d2i.index(node), side="right")) - 1
                bpc = c.plan()["bpc"]
                assert blk(f["x"]) == f["block"] and blk(f["d"]) == f["block"] + 1 and f["block"] // bpc == (f["block"] + 1) // bpc
                anc = f["d"]
                while anc > 0 and anc != f["x"]:
                    anc = int(c.tree.parent[anc])
                assert anc == f["x"] and [m[0] for m in c.info.muts(f["x"])][-1] == q
                assert c.tree.mut_pos.tolist().count(q) == 1
            (r, moved), = f["moved"].items()
            pos = [[e[0] for e in l] for l in lists]
            if tag == "a":
                assert q in pos[r] and q + H in pos[r]
            else:
                assert q in pos[r - 1] and q + H not in pos[r - 1] and q + H in pos[r] and q not in pos[r]
            # the word at q + 2^19, read as a word at q, changes the read's answer: confusing the two cannot pass by luck
            ot = oracle.OracleTree(c.tree)
            assert _answers(ot, [lists[r]]) != _answers(ot, [moved])
            if dense:
                assert _answers(ot, [lists[r]])[0][1] == _answers(ot, [moved])[0][1]      # (both on D; the scores differ)
            assert [e for e in moved if e[0] == q][0][1:] == [e for e in lists[r] if e[0] == q + H][0][1:]
        e = sc.CASES["pos_e_%s" % kind]()
        assert sum(1 for l in e.lists() if l[-1][0] == (1 << 20) - 2) == 1 and e.plan()["dense"] == dense
        f = sc.CASES["pos_f_%s" % kind]()
        ff, lists = f.facts, f.lists()
        assert ff["listing_q"] == 0 and sum(1 for l in lists if any(x[0] == ff["twin"] for x in l)) == 1
        assert ff["twin"] > f.info.max_pos and ff["twin"] % (32 * f.info.bm_words) == ff["q"] and f.info.blocks_of(ff["q"])
    for kind, k in (("plain", 5), ("long", 18)):
        for tag, last, dense in (("c_below", H - 2, 1), ("c", H - 1, 0), ("d", H, 0)):
            c = sc.CASES["pos_%s_%s" % (tag, kind)]()
            f = c.facts
            assert f["max_pos"] == f["last"] == last and c.plan()["dense"] == (dense if k >= 16 else 0) and (_k(c) == k).all()
            n_ent, n2 = f["n_ent"]
            assert n_ent < n2 and len(f["listing_last"]) >= 2 and 2 in f["listing_last"]      # padding keys behind the real ones
            assert f["leaf_word"][2] != f["leaf_word"][1] and f["block"] in c.info.blocks_of(last)
            if k >= 16:
                assert f["hits_in_block"] >= sc.DENSE_MIN_HITS


def test_block_and_chunk_cases():
    for name, k in (("heavy_block_plain", 5), ("heavy_block_dense", 18), ("heavy_block_window", 40)):
        c = sc.CASES[name]()
        f = c.facts
        over = f["over_w1"] if c.window is not None else f["over"]
        assert len(over) == 2 and (_k(c) == k).all()             # the heavy node's enter events, and its exit events
        for b, tail in over.items():
            assert set(f["keep"]) <= set(tail), (name, b)        # the reads list positions among the events behind the 128th
        assert sum(1 for l in c.lists() if set(f["keep"]) <= set(e[0] for e in l)) >= 6
        if c.window is not None:
            lo = c.window * sc.WIN_STRIDE
            assert all(lo <= l[0][0] and l[-1][0] < lo + sc.WIN_SIZE for l in c.lists()) and k > sc.WIN_MIN_ENTRIES
            assert c.plan()["key_cap"] == lo and c.plan()["kind"] == "window"
    for nb in sc.CHUNK_TREES:
        c = sc.CASES["chunk_%d" % nb]()
        p = c.plan()
        assert (p["NB"], p["bpc"], p["nchunks"], p["T"], p["dense"]) == (nb, nb, 1, 1, 0)
        assert p["ntiles"] == c.reads.n_reads >= 4096 >= sc.SORT_MIN_READS and _k(c).min() >= 1
    assert sorted(sc.CHUNK_TREES) == [59, 60, 61, 121]           # below, at and above one group of 60 blocks; 2 groups + 1


def test_finalize_cases(oracle):
    for nchunks, counts in sc.FINALIZE_COUNTS.items():
        c = sc.CASES["finalize_%d" % nchunks]()
        assert c.counts == counts and c.reads.n_reads == max(counts) and _k(c).max() < 16
        for n in counts:
            assert c.plan(n)["nchunks"] == nchunks and c.plan(n)["dense"] == 0
        # read counts on both sides of a workgroup's share
        per = sc.finalize_reads_per_workgroup(nchunks)
        if len(counts) == 2:
            assert counts == (per, per + 1)
    assert sc.CASES["finalize_129"]().info.flat.cp_stride == 2
    assert [sc.finalize_lanes_per_read(n) for n in sorted(sc.FINALIZE_COUNTS)] == [1, 4, 4, 16, 16, 64]
    one = sc.CASES["finalize_one_chunk"]()
    p = one.plan()
    assert p["nchunks"] >= 9 and sc.finalize_lanes_per_read(p["nchunks"]) == 4
    ot = oracle.OracleTree(one.tree)
    d2b = one.info.flat.get("dfs2bfs")
    n0 = one.info.flat.get("blk_node0")
    for l in one.lists():
        cols = list(zip(*l))
        ns = ot.place_sample(*cols, per_node_scores=True)["node_scores"]
        root = int(ns[0])
        within = np.flatnonzero(np.asarray(ns)[d2b] <= root + 1)          # DFS indices of the nodes within the bound
        assert len(within) >= 1 and within.max() < n0[p["bpc"]], "a node within the bound outside the first chunk"


def _in_window(l, window):
    lo = window * sc.WIN_STRIDE
    return lo <= l[0][0] < lo + sc.WIN_STRIDE and l[-1][0] < lo + sc.WIN_SIZE and len(l) > sc.WIN_MIN_ENTRIES


def test_window_table_cases():
    for name in ("win_64_65_words", "win_tiles", "win_first_and_last_position", "win_pair_rounds", "heavy_block_window"):
        c = sc.CASES[name]()
        assert all(_in_window(l, c.window) for l in c.lists()), name
        # (every finite bound of the tree-wide streams lies below root score + words: the read's only crown is the window's)
        taus = [int(t) for t in c.info.flat.stats.stream_tau[:c.info.flat.n_streams - 1]]
        assert all(sm.theta(c.info.flat, l) > max(taus) for l in c.lists()), name
        p = c.plan()
        assert p["kind"] == "window" and p["dense"] == 1 and p["key_cap"] == c.window * sc.WIN_STRIDE
    assert sorted(sc.CASES["win_64_65_words"]().facts["k"]) == [33, 40, 64, 64, 65, 65, 65]
    t = sc.CASES["win_tiles"]()
    assert t.counts == (31, 32, 33, 64) and all(t.plan(n)["ntiles"] == 1 for n in t.counts)
    e = sc.CASES["win_first_and_last_position"]()
    f = e.facts
    assert (f["first"], f["last"]) == (e.window * sc.WIN_STRIDE, e.window * sc.WIN_STRIDE + sc.WIN_SIZE - 1) and e.info.max_pos == f["last"]
    assert f["listing"] == [7, 7] and f["leaf_word"][2] != f["leaf_word"][1] and e.info.blocks_of(f["first"], "w1") and e.info.blocks_of(f["last"], "w1")
    o = sc.CASES["win_just_outside"]()
    assert o.window is None and o.facts["outside"] == e.facts["last"] + 1 == o.info.max_pos and o.facts["listing"] == [6, 6]
    assert all(not _in_window(l, 1) and _in_window(l[:-1], 1) for l in o.lists()) and o.plan()["kind"] == "sweep" and o.plan()["dense"] == 1
    r = sc.CASES["win_pair_rounds"]()
    f = r.facts
    assert f["listing"] == [64, 64] and f["pairs"] > 128 and f["crossing"] >= 1 and r.reads.n_reads == 64
    assert all(f["block"] in r.info.blocks_of(p, "w0") for p in f["keep"])


def test_arena_cases():
    for nb, (n_nodes, wi, ci) in sc.ARENA_CROWNS.items():
        c = sc.CASES["arena_%d" % nb]()
        f = c.facts
        assert c.tree.n_nodes == n_nodes and f["NB"] == nb and c.arena == (wi, ci)
        assert [sc.window_crown_of(c.info, l) for l in c.lists()] == [(wi, ci)] * 6
        assert all(sc.WALK16_K < k <= sc.WIN_MIN_ENTRIES for k in f["k"]) and {17, 32} <= set(f["k"])
        assert f["chunks_used"] == {1: 1, 15: 15, 16: 16, 17: 9}[nb] and f["bpc"] == (2 if nb == 17 else 1)


# ---- every case on a small tree through the model of the sweep -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in sc.CASES if not n.startswith(("finalize_1", "finalize_3", "chunk_"))))
def test_model_of_the_sweep_on_the_cases(oracle, name):
    c = sc.CASES[name]()
    assert c.tree.n_nodes <= 12000
    lists = c.lists()
    pick = sorted(set(c.facts.get("special", [])) | set(range(min(4, len(lists)))) | set(range(len(lists) - 2, len(lists))))
    pick = [r for r in pick if len(lists[r]) <= 200]
    ot = oracle.OracleTree(c.tree)
    want = _answers(ot, [lists[r] for r in pick])
    # the stream the device sweeps for the case: the whole tree, the window's stream, or the reads' window crown
    stream = "c%d.%d" % c.arena if c.arena else "w%d" % c.window if c.window is not None else None
    fm = sm.FlatModel(c.info.flat, stream)
    nchunks = sc.ARENA_CHUNKS if c.arena else c.plan()["nchunks"]
    for r, exp in zip(pick, want):
        got = fm.place_full(lists[r], nchunks=nchunks)
        assert (got["score"], got["best_j"], got["num_best"], got["has_unique"]) == exp, (name, r)


# ---- the library's planner on the cases, without a GPU ----------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STREAMS, MAX_WINDOWS = 16, 32          # flatmat.hpp
PLAN_SWEEP, PLAN_WIN_BASE, WC_SLOT = 2, 5 * MAX_STREAMS, MAX_STREAMS - 1      # device_mat.hpp: plan id = class * MAX_STREAMS + stream
PLAN_SEED_ID = PLAN_WIN_BASE + MAX_WINDOWS
WEPP_EDEVICE, WEPP_ELIMIT = 3, 4           # include/wepp_place.h


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def planner(request, tmp_path_factory):
    """tests/cxx/launch_plan_main.cpp built against the emulated runtime's headers, plain and under ASan + UBSan."""
    tmp = tmp_path_factory.mktemp("launch_plan_" + request.param)
    flags = ["-O1"]
    if request.param == "sanitized":
        probe = tmp / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        can = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
        if can.returncode != 0:
            pytest.skip("no sanitizer runtime: " + can.stderr[-200:])
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp / "launch_plan_main")
    srcs = [os.path.join(ROOT, "tests", "cxx", "launch_plan_main.cpp"), os.path.join(ROOT, "wepp_amd", "csrc", "errors.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", *flags, "-I", os.path.join(ROOT, "tests", "cxx", "hip_emu"),
                            *srcs, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]

    def run(T, tree, streams, wstreams, triples, walking=0, fuse_windows=1):
        """tree = (bm_words, max_pos, seed_chunks, wc_windows); streams / wstreams: geometries; triples: (plan id, count, maxk)."""
        geo = lambda g: "%d %d %d %d" % (g["NB"], g["ncp"], g["cp_stride"], g["sbytes"])
        text = "\n".join(["%d %d %d" % (T, walking, fuse_windows), "%d %d %d %d %d" % (tree[0], tree[1], len(streams), tree[2], tree[3])] + [geo(g) for g in streams]
                         + [str(len(wstreams))] + [geo(g) for g in wstreams] + [str(len(triples))] + ["%d %d %d" % t for t in triples]) + "\n"
        return subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    return run


def _problem(c, count):
    """The planning problem of the call that places the first `count` reads of a tile case: its one plan id with the
    case's geometry on the stream that id names (the other streams are never asked about)."""
    maxk = int(max(1, _k(c)[:count].max()))
    tree = (c.info.bm_words, c.info.max_pos, 0, 0)
    ns = int(c.info.flat.n_streams)
    none = dict(NB=1, ncp=1, cp_stride=1, sbytes=0)
    if c.window is None:
        return tree, [none] * (ns - 1) + [sc.stream_geometry(c.info.flat)], [], [(PLAN_SWEEP * MAX_STREAMS + ns - 1, count, maxk)]
    return tree, [none] * ns, [none] * c.window + [sc.stream_geometry(c.info.flat, "w%d" % c.window)], [(PLAN_WIN_BASE + c.window, count, maxk)]


TILE_CASES = sorted(n for n in sc.CASES if not n.startswith("arena_"))


def test_every_case_without_a_plan_line_is_an_arena_case():
    assert all((sc.CASES[n]().arena is None) == (n in TILE_CASES) for n in sc.CASES) and len(TILE_CASES) == len(sc.CASES) - len(sc.ARENA_CROWNS)


def _plan_output(text):
    """(`[plan]` lines parsed, the `[launch]` line as a dict: the partition as index lists, the totals as numbers)."""
    rows = text.splitlines()
    assert rows and rows[-1].startswith("[launch] ") and all(r.startswith("[plan] ") for r in rows[:-1]), text
    launch = {}
    for kv in rows[-1].split()[1:]:
        k, v = kv.split("=")
        launch[k] = [int(x) for x in v.split(",") if x] if k in ("plain", "windows", "others") else v if "@" in v else int(v)
    return [sc.parse_plan_line(r) for r in rows[:-1]], launch


def test_planner_on_several_plans(planner):
    """A call with a dense plan on stream 2, a plain one on the whole tree, window-crown sweeps and a table window plan:
    the plans in plan-id order, each behind the partials of those before it, the arena's between; the partition with the
    window plans fused and not; passes = tiles + arena reads, bytes = tiles x stream bytes (no walks in the call)."""
    small, whole, win = dict(NB=40, ncp=40, cp_stride=1, sbytes=20000), dict(NB=300, ncp=150, cp_stride=2, sbytes=3 << 20), dict(NB=26, ncp=26, cp_stride=1, sbytes=9000)
    max_pos, ns = 2000, 7
    triples = [(PLAN_SWEEP * MAX_STREAMS + 2, 10, 18), (PLAN_SWEEP * MAX_STREAMS + ns - 1, 70, 5), (PLAN_SWEEP * MAX_STREAMS + WC_SLOT, 6, 20), (PLAN_WIN_BASE + 1, 70, 40)]
    for fuse in (1, 0):
        run = planner(64, (64, max_pos, 0, 1), [small] * (ns - 1) + [whole], [win, win], triples, fuse_windows=fuse)
        assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
        lines, launch = _plan_output(run.stdout)
        want = [sc.predict_plan(10, 18, small, max_pos), sc.predict_plan(70, 5, whole, max_pos),
                sc.predict_plan(70, 40, win, max_pos, window=1, win_tiles=2 if fuse else None)]
        assert [{k: l[k] for k in sc.PLAN_FIELDS} for l in lines] == want, (fuse, lines, want)
        assert [l["t"] for l in lines] == [2, ns - 1, ns - 1] and [l["off"] for l in lines] == [0, 10, 86]
        size = [12 * w["nchunks"] * w["count"] for w in want]
        arena_part = size[0] + size[1]
        assert [l["part_off"] for l in lines] == [0, size[0], arena_part + 12 * sc.ARENA_CHUNKS * 6], (fuse, lines)
        assert launch["arena"] == "6@%d" % arena_part and launch["part_total"] == sum(size) + 12 * sc.ARENA_CHUNKS * 6 and launch["seeds"] == 0
        assert (launch["plain"], launch["windows"], launch["others"]) == (([1], [2], [0]) if fuse else ([1], [], [0, 2])), (fuse, launch)
        assert launch["passes"] == sum(w["ntiles"] for w in want) + 6 and launch["walk_reads"] == 0
        assert launch["bytes"] == sum(w["ntiles"] * g["sbytes"] for w, g in zip(want, (small, whole, win)))


@pytest.mark.parametrize("name", TILE_CASES)
def test_planner_on_the_cases(planner, name):
    c = sc.CASES[name]()
    for count in c.counts:
        tree, streams, wstreams, triples = _problem(c, count)
        run = planner(c.knobs["tile"], tree, streams, wstreams, triples)
        assert run.returncode == 0, (name, count, run.stdout[-500:], run.stderr[-2000:])
        lines, launch = _plan_output(run.stdout)
        assert len(lines) == 1, (name, count, run.stdout)
        assert {k: lines[0][k] for k in sc.PLAN_FIELDS} == c.plan(count), (name, count, lines[0], c.plan(count))
        # the one plan: at the front of the partials, in the part of the partition its kind belongs to
        kind = "windows" if c.window is not None and lines[0]["dense"] else "others" if lines[0]["dense"] or not lines[0]["ent_cap"] else "plain"
        assert lines[0]["part_off"] == 0 and launch["part_total"] == 12 * lines[0]["nchunks"] * count, (name, count, run.stdout)
        assert {k: launch[k] for k in ("plain", "windows", "others")} == {k: [0] if k == kind else [] for k in ("plain", "windows", "others")}, (name, launch)
        assert launch["passes"] == lines[0]["ntiles"], (name, launch)


def test_planner_errors(planner):
    g = dict(NB=64, ncp=64, cp_stride=1, sbytes=30000)
    for what, tree, triples, code, message in (
            ("a plan id beyond the window plans' and the seeds'", (64, 2000, 0, 0), [(PLAN_SEED_ID + 1, 5, 5)], WEPP_EDEVICE, "routing produced an invalid plan id"),
            ("PLAN_SEED on a handle without signatures", (64, 2000, 0, 0), [(PLAN_SEED_ID, 5, 70)], WEPP_EDEVICE, "routing produced an invalid plan id"),
            ("count * ARENA_CHUNKS at 2^31", (64, 2000, 0, 1), [(PLAN_SWEEP * MAX_STREAMS + WC_SLOT, (1 << 31) // sc.ARENA_CHUNKS, 20)], WEPP_ELIMIT,
             "too many window-crown sweeps in one call; split the batch")):
        run = planner(64, tree, [g] * 7, [g], triples)
        assert run.returncode == 3 and run.stdout == "error %d: %s\n" % (code, message), (what, run.stdout, run.stderr[-2000:])
    # (one below the limit plans)
    run = planner(64, (64, 2000, 0, 1), [g] * 7, [g], [(PLAN_SWEEP * MAX_STREAMS + WC_SLOT, (1 << 31) // sc.ARENA_CHUNKS - 1, 20)])
    assert run.returncode == 0 and _plan_output(run.stdout)[0] == [], (run.stdout, run.stderr[-2000:])
