"""tests/seed_cases.py held to its edges on the CPU, by the model of k_seed (tests/seed_model.py) and the oracle only:
for every builder the fact about its INPUT that makes it an edge case -- hit events per group and block against
64 / 96 / 97, groups of 32 blocks and tails, rounds of 512 events, nh and |T|, a byte counter at 255, levels of 255 and
256 chunks, the level a sample is handed over at, exact chunk counts, optimal nodes in chunks that different waves,
passes and parts evaluate.  A builder that drifts cannot hollow a case out unnoticed.  The constants the model restates
are read from the sources: a changed constant fails here, the edge does not move silently."""
import os
import re

import numpy as np
import pytest

import fuzz_trees as ft
import seed_cases as sc
import seed_model as sdm
import wepp_amd as w

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wepp_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _const(text, name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


# ---- the constants -----------------------------------------------------------------------------------------------------
def test_restated_constants_match_the_sources():
    kern, dev, flat = _src("seed_kernels.hip"), _src("device_mat.hpp"), _src("flatmat.hpp")
    assert _const(kern, "SEED_HIT_CAP") == sdm.SEED_HIT_CAP == 96
    assert _const(dev, "SEED_MAX_HARD") == sdm.SEED_MAX_HARD == 255
    assert _const(dev, "SEED_HEAVY_LEVEL_MIN") == sdm.SEED_HEAVY_LEVEL_MIN == 256
    assert _const(dev, "SEED_HEAVY_PARTS") == sdm.SEED_HEAVY_PARTS == 32
    assert _const(dev, "SEED_HEAVY_CAP") == sdm.SEED_HEAVY_CAP == 128
    assert _const(dev, "SEED_MAX_ENTRIES") == sdm.SEED_MAX_ENTRIES == 4096
    assert _const(dev, "SEED_MIN_HARD") == sdm.SEED_MIN_HARD == 3
    assert int(re.search(r"#define WEPP_SEED_THREADS (\d+)", dev).group(1)) == sdm.SEED_THREADS
    assert _const(flat, "SEED_CHUNK_BLOCKS") == sdm.SEED_CHUNK_BLOCKS == 16
    assert int(re.search(r"#define WEPP_WIN_SIZE (\d+)", flat).group(1)) == sc.WIN_SIZE
    assert int(re.search(r"#define WEPP_WIN_STRIDE (\d+)", flat).group(1)) == sc.WIN_STRIDE
    # the 32-block group, the 8 x 64 scan round, the slab of 64 chunks
    assert re.search(r"bg \+= (\d+)\)", kern).group(1) == str(sdm.GROUP_BLOCKS)
    assert re.search(r"ng = min\((\d+)u, b1 - bg\)", kern).group(1) == str(sdm.GROUP_BLOCKS)
    assert re.search(r"e \+= (\d+) \* (\d+)\)", kern).groups() == ("8", "64") and sdm.SCAN_ROUND == 512
    assert re.search(r"s0 \+= (\d+) \* SEED_WAVES", kern).group(1) == str(sdm.SLAB)
    # seed_lds_bytes as the model restates it
    assert "(m.bm_words + ent_cap + (SEED_MAX_HARD + 1) + seed_h_words(m.seed_chunks) + SEED_SHARED_WORDS + SEED_WAVES * 3 * SEED_HIT_CAP) * 4" in kern
    assert "SEED_SHARED_WORDS = 16 + 3 * SEED_WAVES" in kern and "return ((chunks + 63) & ~63u) / 4" in kern
    assert sdm.seed_lds_bytes(128, 64, 13) == (128 + 64 + 256 + 16 + 40 + 2304) * 4
    assert [sdm.seed_h_words(n) for n in (1, 64, 65, 512, 513)] == [16, 16, 32, 128, 144]


# ---- the model itself --------------------------------------------------------------------------------------------------
def test_optimal_nodes_lie_in_must_chunks_on_the_fuzz_trees(oracle, monkeypatch):
    """The trees and samples of test_seed_model.test_seed_bound_fuzz: the extended model's bound is the old one, the
    oracle's optimal nodes all lie in `must` chunks, and the level counts add up."""
    monkeypatch.setenv("WEPP_SEED_CHUNK_BLOCKS", "1")
    rng = np.random.default_rng(41)
    seen = 0
    for it in range(150):
        genome = int(rng.choice([20, 200, 1500]))
        tree, ref = ft.random_tree(rng, n_nodes=int(rng.integers(2, 400)), genome=genome, p_masked=0.04, p_ambig=0.12)
        m = sdm.SeedModel(w.FlatView(tree))
        ot = oracle.OracleTree(tree)
        for _ in range(4):
            S = ft.random_sample(rng, ref, genome=genome, max_k=int(rng.integers(0, 24)))
            if rng.random() < 0.3:
                S = S + [(genome + 5, 1, 2, 0)]
            o = ot.place_sample(*(list(zip(*S)) if S else ([], [], [], [])), per_node_scores=True, want_best_vec=True)
            H, sT, nh = m.counts(S)
            assert (sT - H == m.lower_bounds(S)).all() and nh == len(m.hard_entries(S)[0])
            Hl, cnt = m.levels(S)
            assert cnt.sum() == m.nch and (Hl == H).all()
            best, root = int(o["score"]), int(o["node_scores"][0])
            must, may = m.must_may(S, best, root)
            assert 1 <= must <= may <= m.nch
            for j in o["best_j_vec"]:
                assert sT - H[m.chunk_of_bfs(int(j))] <= best, (it, S, int(j))
                seen += 1
            assert m.defer_level(S) in (None, 0) or cnt[m.defer_level(S)] >= sdm.SEED_HEAVY_LEVEL_MIN
        ot.close()
    assert seen > 600


# ---- every case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_every_sample_is_a_whole_genome_sample(name):
    """What routing needs of a seeded sample: no genome window holds it (or it lies beyond all of the tree's windows),
    at most SEED_MAX_ENTRIES entries, ascending positions; the trees are in DFS pre-order."""
    c = sc.CASES[name]()
    assert (c.flat.info.flat.get("dfs2id") == np.arange(c.tree.n_nodes)).all()
    assert c.model.cp_stride == 1 and c.model.stride == c.stride and c.model.n_cp == c.model.nb
    n_win = (c.model.max_pos + sc.WIN_STRIDE) // sc.WIN_STRIDE
    for n in c.names:
        S = c.samples[n]
        assert [e[0] for e in S] == sorted(set(e[0] for e in S)), n
        if n in c.seeded:
            assert len(S) <= sdm.SEED_MAX_ENTRIES
            assert not sc.in_one_window(S) or S[0][0] // sc.WIN_STRIDE >= n_win, n


def _all_groups(m, S):
    return [g for c in range(m.nch) for g in m.group_hits(S, c)]


def _in_must(c, ex, S, chunk):
    H, sT, _ = c.model.counts(S)
    return sT - H[chunk] <= ex["best"]


def test_hit_list_edges_in_one_block(oracle):
    """SEED_HIT_CAP and apply_hits' rounds of 64, one block per chunk: 63 / 64 / 65 / 96 hit events in one block are
    listed (no group of the sample overflows), 97 and a whole block of 128 take the block-by-block path."""
    c = sc.CASES["hits_one_block"]()
    ex = sc.expectations(c, oracle)
    b = c.facts["chunk"]
    assert c.stride == 1 and c.facts["targets"] == dict(h63=63, h64=64, h65=65, h96=96, h97=97, hall=128)
    for n, h in c.facts["targets"].items():
        S = c.samples[n]
        (g,) = c.model.group_hits(S, b)
        assert g["blocks"] == 1 and g["hits"] == h and g["per_block"] == [h], n
        assert _in_must(c, ex[n], S, b), n                       # the block is evaluated, whatever the waves' order
        worst = max(x["hits"] for x in _all_groups(c.model, S))
        assert worst == h, n
        assert (worst > sdm.SEED_HIT_CAP) == (n in ("h97", "hall")), n
    assert 64 < 65 <= sdm.SEED_HIT_CAP < 97


@pytest.mark.parametrize("stride", [32, 33, 40])
def test_group_edges(oracle, stride):
    """Groups of exactly 32 blocks (lane 32 loads the group's end offset), tail groups, a chunk cut short by the end of
    the tree; 96 / 97 hit events spread over a group's blocks; more than 512 events with hits in both rounds."""
    c = sc.CASES["groups_%d" % stride]()
    m = c.model
    ex = sc.expectations(c, oracle)
    assert c.stride == stride and m.nb == 55 and m.nch == 2
    shape = [[g["blocks"] for g in m.group_hits([], ch)] for ch in range(m.nch)]
    assert shape == {32: [[32], [23]], 33: [[32, 1], [22]], 40: [[32, 8], [15]]}[stride]       # ng == 32, a tail group, a short chunk
    for n, (ch, g, h) in c.facts["targets"].items():
        S = c.samples[n]
        gh = m.group_hits(S, ch)[g]
        assert gh["hits"] == h and _in_must(c, ex[n], S, ch), n
        if h <= sdm.SEED_HIT_CAP:
            assert max(x["hits"] for x in _all_groups(m, S)) <= sdm.SEED_HIT_CAP, n       # no group of the sample overflows
        if gh["blocks"] > 1:
            assert sum(1 for x in gh["per_block"] if x) >= min(8, (gh["blocks"] + 1) // 2), n          # spread over the group's blocks
        if n.startswith("rounds_"):
            assert gh["events"] > sdm.SCAN_ROUND and len(gh["rounds"]) >= 2 and gh["rounds"][0] >= 20 and gh["rounds"][-1] >= 20, n
    t = c.facts["targets"]
    assert {h for (_, _, h) in t.values()} == {80, 96, 97, 140}
    assert (0, 0, 96) in t.values() and (0, 0, 97) in t.values() and (1, 0, 96) in t.values()
    if stride > 32:
        assert (0, 1, 96) in t.values() and (0, 1, 97) in t.values()


def test_hard_entry_edges(oracle):
    """SEED_MAX_HARD, the SWAR flush at 15, the byte counter at 255, max_pos and beyond, nh == 0, |T| == 0."""
    c = sc.CASES["hard_entries"]()
    m = c.model
    ex = sc.expectations(c, oracle)
    cx = m.chunk_of_dfs(1)                                     # X's chunk
    assert m.max_pos == sc.HARD_GENOME and m.sig.shape[0] == m.max_pos + 2
    over = sc.CASES["hard_over"]()
    assert over.key == c.key and over.env == c.env and over.over_max_hard() and not c.over_max_hard()
    for h in sc.HARD_COUNTS:
        S = (c if h <= 255 else over).samples["hard_%d" % h]
        inside, beyond = m.hard_entries(S)
        H, sT, nh = m.counts(S)
        assert len(inside) == h and beyond == 0 and nh == min(h, 255) == sT
        assert H.max() == min(h, 255) == H[cx], h              # all served by one chunk's signature (X's and the chunks below X)
        assert sc.expectations(c if h <= 255 else over, oracle)["hard_%d" % h]["root"] == h
    assert set(sc.HARD_COUNTS) >= {14, 15, 16, 30, 31, 254, 255, 256, 300}
    H255 = m.counts(c.samples["hard_255"])[0]
    assert (H255 == 255).sum() >= 1 and m.levels(c.samples["hard_255"])[1][255] >= 1     # byte counter = 255, lvl[255]
    assert len(m.hard_entries(c.samples["hard_255"])[0]) == sdm.SEED_MAX_HARD
    _, sT, nh = m.counts(c.samples["hard_255_beyond"])
    assert (nh, sT) == (255, 258)
    _, sT, nh = m.counts(over.samples["hard_300_beyond"])
    assert (nh, sT) == (255, 256)
    S = c.samples["at_max_pos"]
    inside, beyond = m.hard_entries(S)
    assert any(p == m.max_pos for p, _ in inside) and any(e[0] == m.max_pos + 1 for e in S) and beyond == 2
    assert m.counts(S)[0][m.nch - 1] >= 1 and m.nibble(m.max_pos, m.nch - 1)            # the last signature row serves it
    H, sT, nh = m.counts(c.samples["all_beyond"])
    assert (nh, sT, H.max()) == (0, 3, 0) and len(c.samples["all_beyond"]) == 5
    H, sT, nh = m.counts(c.samples["no_hard"])
    assert (nh, sT, H.max()) == (0, 0, 0) and m.levels(c.samples["no_hard"])[1][0] == m.nch
    assert ex["no_hard"]["must"] == ex["no_hard"]["may"] == m.nch
    # |T| counts the entries beyond the tree: the sample is a node's genotype plus three of them, the optimum (3) is
    # found at the top level, and only chunks that serve ALL its hard entries inside the tree are evaluated
    S = c.samples["node_beyond"]
    H, sT, nh = m.counts(S)
    e = ex["node_beyond"]
    assert sT == nh + 3 and e["best"] == 3 and e["settled"] and nh >= 5
    assert e["must"] == int((H == nh).sum()) < int((H >= nh - 3).sum()) <= e["may"]


@pytest.mark.parametrize("nch", sc.NCH)
def test_chunk_count_edges(oracle, nch):
    """Exactly nch chunks: the byte counters' words, the signature rows rounded to four words, the guard of the last
    counter word, the last slab of 64; the last chunk holds an optimal node; ties across slabs (and parts)."""
    c = sc.CASES["nch_%d" % nch]()
    m = c.model
    ex = sc.expectations(c, oracle)
    assert m.nch == m.nb == nch and c.stride == 1
    assert m.row_words == (((nch + 7) // 8) + 3) & ~3
    a, b = ex["tie_a"], ex["tie_b"]
    assert (a["best"], a["root"]) == (1, 1) and (b["best"], b["root"]) == (0, 0)
    assert 0 in a["chunks"] and 0 in b["chunks"] and nch - 1 in b["chunks"] and nch - 1 in a["chunks"]      # the root's chunk and the LAST one tie
    assert m.counts(c.samples["tie_b"])[1] == 0 and b["must"] == b["may"] == nch         # every chunk is evaluated: nch of them
    assert m.counts(c.samples["tie_a"])[0][0] == 0                               # (no twin in chunk 0)
    if nch > sdm.SLAB:
        assert len(set(ch // sdm.SLAB for ch in a["chunks"])) >= 2 and len(set(ch // sdm.SLAB for ch in b["chunks"])) >= 2
        assert a["num_best"] >= 3
    for n in c.names:
        if n.startswith("node_in_chunk_"):
            ch = int(n.rsplit("_", 1)[1])
            assert ch in ex[n]["chunks"] and ex[n]["best"] < ex[n]["root"], n
    assert "node_in_chunk_%d" % (nch - 1) in c.names and "node_in_chunk_0" in c.names
    lvl = m.defer_level(c.samples["tie_b"])
    assert c.deferral == (nch >= sdm.SEED_HEAVY_LEVEL_MIN) == (lvl == 0)
    if nch > sdm.SLAB * (sdm.SEED_THREADS // 64):
        # handed over at the top level on a tree of more than 512 chunks: two PARTS of the second pass hold the tie
        assert min(b["chunks"]) < 512 <= max(b["chunks"])


def test_level_edges(oracle):
    """SEED_HEAVY_LEVEL_MIN: a level of 255 chunks stays, one of 256 is handed over -- at the top level (the first pass
    evaluates nothing) or below it (the first pass hands over the score it found, and the tie continues below)."""
    c255, c256, low = sc.CASES["defer_255"](), sc.CASES["defer_256"](), sc.CASES["defer_lower"]()
    assert (c255.model.nch, c256.model.nch, low.model.nch) == (255, 256, 400)
    assert c255.model.levels(c255.samples["tie_b"])[1][0] == 255 and c255.model.defer_level(c255.samples["tie_b"]) is None
    assert c255.model.defer_level(c255.samples["tie_a"]) is None and not c255.deferral
    H, cnt = c256.model.levels(c256.samples["tie_b"])
    assert cnt[0] == 256 and H.max() == 0 and c256.model.defer_level(c256.samples["tie_b"]) == 0        # defer_level == hmax
    H, cnt = c256.model.levels(c256.samples["tie_a"])
    assert H.max() == 1 and 0 < cnt[1] < 256 and 0 < cnt[0] < 256 and c256.model.defer_level(c256.samples["tie_a"]) is None
    # below the top level: level 1 (the twins' chunks) belongs to the first pass and holds optimal nodes, level 0 is
    # reached (|T| - 0 = 1 <= the optimum) and holds the root, which ties
    S = low.samples["tie_a"]
    H, cnt = low.model.levels(S)
    e = sc.expectations(low, oracle)["tie_a"]
    assert H.max() == 1 and low.model.defer_level(S) == 0 and 0 < cnt[1] < 256 <= cnt[0]
    assert e["best"] == 1 and low.model.counts(S)[1] == 1 and e["must"] == 400
    above = [ch for ch in e["chunks"] if H[ch] == 1]
    below = [ch for ch in e["chunks"] if H[ch] == 0]
    assert len(above) >= 2 and 0 in below
    assert low.model.defer_level(low.samples["tie_b"]) == 0
    # the table of the second pass: 128 samples fill it, the 129th stays with its own workgroup
    cap = sc.CASES["heavy_cap"]()
    assert cap.counts == (sdm.SEED_HEAVY_CAP, sdm.SEED_HEAVY_CAP + 1) == (128, 129) and len(cap.names) == 129
    assert all(cap.model.defer_level(S) == 0 for S in cap.lists()) and len(set(map(tuple, cap.lists()))) == 129
    assert cap.key == c256.key and cap.env == c256.env               # (the same handle)


def test_routing_edges():
    """k <= SEED_MAX_ENTRIES, n_hard >= SEED_MIN_HARD, a one-entry sample beside a 4096-entry one."""
    c = sc.CASES["route_entries"]()
    k = {n: len(c.samples[n]) for n in c.names}
    assert k == dict(one=1, k4096=4096, k4097=4097, k100=100) and c.seeded == {"one", "k4096", "k100"}
    assert (max(k[n] for n in c.seeded) + 63) & ~63 == 4096
    assert max(x["hits"] for x in _all_groups(c.model, c.samples["k4096"])) > sdm.SEED_HIT_CAP
    r = sc.CASES["route_min_hard"]()
    hard = {n: sum(len(x) if isinstance(x, list) else x for x in r.model.hard_entries(r.samples[n])) for n in r.names}
    assert hard == dict(hard_2=2, hard_3=3, hard_4=4) and r.seeded == {"hard_3", "hard_4"}
    assert r.env["WEPP_SEED_MIN_HARD"] is None and all(len(S) == 6 for S in r.lists())
    assert all(cc().env["WEPP_SEED_MIN_HARD"] == "0" for n, cc in sc.CASES.items() if n != "route_min_hard")


def test_ties_between_waves_passes_and_parts(oracle):
    """The optimum attained in chunks of different slabs of 64 (different waves), above and below the level a sample
    is handed over at (first and second pass), and in chunks that different parts of the second pass take."""
    waves = sc.expectations(sc.CASES["nch_65"](), oracle)["tie_a"]["chunks"]
    assert min(waves) < 64 <= max(waves)
    parts = sc.expectations(sc.CASES["nch_513"](), oracle)["tie_b"]["chunks"]
    assert min(parts) < 512 <= max(parts)
    low = sc.CASES["defer_lower"]()
    H = low.model.counts(low.samples["tie_a"])[0]
    lv = sorted(set(int(H[ch]) for ch in sc.expectations(low, oracle)["tie_a"]["chunks"]))
    assert lv == [0, 1] and low.model.defer_level(low.samples["tie_a"]) == 0
