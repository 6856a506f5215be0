"""Every builder of tests/epp_cases.py shows the edge of wepp_epp_map it is for -- checked on the CPU against the
oracle (oracle/epp_oracle.c) and the model in epp_cases.py alone; the library's device code is not run here (only its
tree generator, for one case).  tests/test_epp_map_edges_gpu.py runs the same inputs through wepp_epp_map, so a later
change of a generator cannot hollow those tests out unnoticed."""
from fractions import Fraction

import numpy as np
import pytest

import epp_cases as ec


# ---- the model itself -----------------------------------------------------------------------------------------------
def test_plan_by_hand():
    # 130 reads at one read per lane: tiles of 64, 64, 2 in (start, end, index) order
    start = np.array([5] * 64 + [3] * 64 + [9, 1])
    end = np.array([9] * 64 + [8] * 63 + [4] + [9, 30])
    pl = ec.plan(start, end, 1)
    assert (pl["ntiles"], pl["tpg"], pl["G"]) == (3, 1, 3)
    assert pl["order"][0] == 129 and pl["order"][1] == 127          # [1, 30], then [3, 4] before every [3, 8]
    assert pl["tile_ws"].tolist() == [1, 3, 5] and pl["tile_we"].tolist() == [30, 9, 9]
    # 513 tiles: two tiles per group, the last group holds one
    n = 512 * 64 + 1
    pl = ec.plan(np.arange(n) // 7 + 1, np.arange(n) // 7 + 4, 1)
    assert (pl["ntiles"], pl["tpg"], pl["G"]) == (513, 2, 257) and pl["group_ntiles"].tolist() == [2] * 256 + [1]
    assert pl["group_ws"][1] == pl["tile_ws"][2] and pl["group_we"][1] == pl["tile_we"][3]
    assert ec.plan(np.ones(n), np.ones(n), 4)["tpg"] == 1 and ec.plan(np.ones(4 * n - 3), np.ones(4 * n - 3), 4)["tpg"] == 2


def test_stream_by_hand():
    from wepp_amd import A, C, G, T, Tree
    # ids chosen so that pre-order differs from id order: root 2; its children 0 (leaf) and 1; 1's children 3, 4
    tree = Tree.from_lists([2, 2, -1, 1, 1], [[(7, A, C)], [(5, G, T), (9, A, C)], [], [], [(9, A, C, G), (-1, 0, 0, 0)]])
    dfs2id, dfs_end = ec.preorder(tree)
    assert dfs2id.tolist() == [2, 0, 1, 3, 4] and dfs_end.tolist() == [4, 1, 4, 3, 4]
    st = ec.stream(tree)
    # enter 0 | exit 0, enter 1 (5, 9) | enter 4 | exit 4, exit 1 (5, 9); the masked mutation gives nothing
    assert st["pos"].tolist() == [7, 7, 5, 9, 9, 9, 5, 9]
    assert st["node"].tolist() == [1, 2, 2, 2, 4, 5, 5, 5]
    assert st["exit"].tolist() == [False, True, False, False, False, True, True, True]
    assert st["owner"].tolist() == [1, 1, 2, 2, 4, 4, 2, 2]
    w = ec.window_events(tree, 8, 9)
    assert w["pos"].tolist() == [9, 9, 9, 9] and w["node"].tolist() == [2, 4, 5, 5]
    assert ec.chunks(0) == [(0, 0)] and ec.chunks(1024) == [(0, 1024)] and ec.chunks(1025) == [(0, 1024), (1024, 1025)]


def test_stream_is_the_flatteners():
    """The model's stream against the flattener's own (host code of the library, no device): positions, exit flags and
    node counts, on fuzz trees with masked mutations and on the chunk-cut tree."""
    import fuzz_trees as ft
    import wepp_amd as w
    rng = np.random.default_rng(77)
    trees = [ft.random_tree(rng, genome=60)[0] for _ in range(25)] + [ec.chunk_case("root-2050")["tree"]]
    for tree in trees:
        fv = w.FlatView(tree)
        word, node = fv.get("epp_word"), fv.get("epp_node")
        st = ec.stream(tree)
        assert (word & 0xFFFFF).tolist() == st["pos"].tolist()
        assert ((word >> 30) & 1).astype(bool).tolist() == st["exit"].tolist()
        assert node.tolist() == st["node"].tolist()
        fv.close()


def test_exact_scores_by_hand():
    out = dict(max_parsimony=np.array([0, 2, 1]), multiplicity=np.array([2, 1, 3], np.uint32),
               epp_off=np.array([0, 2, 3, 6], np.uint64), epp_nodes=np.array([0, 3, 3, 0, 1, 3], np.uint32))
    score, n_contrib, deg_sum = ec.exact_scores(out, [3, 5, 7], 4)
    assert score == [Fraction(3, 2) + Fraction(7, 6), Fraction(7, 6), 0, Fraction(3, 2) + Fraction(5, 3) + Fraction(7, 6)]
    assert n_contrib.tolist() == [2, 1, 0, 3] and deg_sum.tolist() == [10, 7, 0, 15]
    assert ec.fx_bits(1023) == 52 and ec.fx_bits(1024) == 51 and ec.fx_bits((1 << 31) - 1) == 31
    assert ec.score_bound(Fraction(1), 4, 1024) == Fraction(4, 2 ** 52) + Fraction(1, 2 ** 51)


# ---- A. chunk cuts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ec.CHUNK_CASES))
def test_chunk_case_shows_its_cuts(oracle, name):
    case = ec.chunk_case(name)
    tree, reads = case["tree"], case["reads"]
    assert (tree.mut_pos >= 0).all() and tree.n_nodes <= ec.ORACLE_LIST_CAP
    # the stated size of the window stream, from window_events
    assert len(ec.window_events(tree, 1, case["genome"])["pos"]) == case["n_events"] == ec.CHUNK_CASES[name][1]
    want = oracle.OracleTree(tree).epp_map(reads, genome_size=case["genome"])
    for rpl in (1, 4):
        shows, pl, gs = ec.chunk_edges(case, want, rpl)
        assert shows == ec.CHUNK_SHOWS[name], (rpl, sorted(shows))
        assert (pl["ntiles"], pl["G"]) == ((3, 3) if rpl == 1 else (1, 1))
        assert len(gs[0]["pos"]) == case["n_events"]
        if rpl == 1:
            assert len(gs[2]["pos"]) == 0          # the third tile's two reads lie behind every mutation: an empty stream
    # the hand-made reads are what they are meant to be
    n = tree.n_nodes
    for r in case["hand"]["everywhere"]:
        assert want["multiplicity"][r] == n
    for r in case["hand"]["last"]:
        assert ec.epp_list(want, r).tolist() == [case["nodes"]["last"]] == [n - 1]
    for r in case["hand"]["first"]:
        assert ec.epp_list(want, r).tolist() == [case["nodes"]["first_a"]]
    r = case["hand"]["under_hub1"][0]
    lst = ec.epp_list(want, r)
    assert lst[0] == case["nodes"]["hub1"] and lst[-1] < case["nodes"]["hub3"] and 50 < len(lst) < case["nodes"]["n_a"]


def test_chunk_cases_cover_every_cut_edge():
    for variant in ("plain", "root"):
        shown = set().union(*(v for k, v in ec.CHUNK_SHOWS.items() if k.startswith(variant)))
        assert shown >= {"one_full_chunk", "spans_chunks", "only_last", "only_first", "open_across_cut", "hub_straddle",
                         "cut_in_pair", "cut_between_nodes"}
    assert "empty_last_chunk" in ec.CHUNK_SHOWS["root-1026"]
    sizes = sorted({v[1] for v in ec.CHUNK_CASES.values()})
    assert sizes == [1024, 1026, 2048, 2050]       # events come in pairs: 1026 and 2050 are the next sizes above


# ---- B. groups of several tiles -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reads", sorted(ec.GROUP_CASES))
def test_group_case_shows_holes(n_reads):
    rpl, tpg, G, last = ec.GROUP_CASES[n_reads]
    case = ec.group_case(n_reads)
    reads = case["reads"]
    assert reads.n_reads == n_reads and len(np.unique(reads.degree)) == 4 and int(reads.degree.sum()) < 2 ** 31
    assert (case["tree"].mut_pos >= 0).all()
    assert ec.effective_rpl(reads.start, reads.end, rpl) == rpl
    e = ec.group_edges(case)
    pl = e["plan"]
    assert (pl["rpl"], pl["tpg"], pl["G"], int(pl["group_ntiles"][-1])) == (rpl, tpg, G, last)
    if n_reads == 32769:
        assert pl["ntiles"] == 513 and n_reads - 512 * 64 == 1      # the last group is one tile of one read
    f = e["found"]
    assert f is not None and e["n_holes"] > 100
    g, t = f["group"], f["tile"]
    assert pl["tile_group"][t] == g and pl["group_ntiles"][g] == tpg
    windows = {(int(pl["tile_ws"][x]), int(pl["tile_we"][x])) for x in range(int(pl["group_tile0"][g]), int(pl["group_tile0"][g]) + tpg)}
    assert len(windows) > 1                                          # tiles of one group with different windows
    assert pl["group_ws"][g] <= f["position"] <= pl["group_we"][g]
    assert not pl["tile_ws"][t] <= f["position"] <= pl["tile_we"][t]
    assert f["position"] in case["tree"].mut_pos
    ev = e["streams"][g]
    m = (ev["pos"][f["block"]:f["block"] + 64] >= pl["tile_ws"][t]) & (ev["pos"][f["block"]:f["block"] + 64] <= pl["tile_we"][t])
    assert m.any() and not m[: int(m.sum())].all()                   # some in the tile, but not a prefix
    assert e["n_empty"] >= 1                                         # and a run with none of its events in the tile


# ---- C. selection ---------------------------------------------------------------------------------------------------
def test_group_skip_case_shows_the_skip():
    case = ec.group_skip_case()
    reads = case["reads"]
    e = ec.skip_edges(case)
    pl = e["plan"]
    assert reads.n_reads == 6 * 64 and pl["G"] == 6 and pl["tpg"] == 1
    assert pl["order"][0] == case["long_read"] and reads.end[case["long_read"]] - reads.start[case["long_read"]] > 0.9 * case["genome"]
    rest = np.delete(np.arange(reads.n_reads), case["long_read"])
    assert (reads.end[rest] - reads.start[rest] < 8).all()
    assert pl["group_we"][0] > pl["group_we"][1] and (np.diff(pl["group_we"][1:]) > 0).all()      # not monotone
    f = e["found"]
    assert f is not None and f["later"] >= 2
    p = f["position"]
    assert p in case["tree"].mut_pos and pl["group_ws"][0] <= p <= pl["group_we"][0]
    assert pl["group_ws"][f["later"]] <= p <= pl["group_we"][f["later"]]
    assert all(not pl["group_ws"][g] <= p <= pl["group_we"][g] for g in range(1, f["later"]))


def test_select_scan_case_needs_the_carry():
    case = ec.select_scan_case()
    n_mut = int((case["tree"].mut_pos >= 0).sum())
    assert n_mut > 131072
    assert ec.select_blocks(case["tree"]) > ec.SEL_SCAN_WIDTH
    assert case["reads"].n_reads == 200
    # a window's events lie on both sides of block 256: without the carry the later blocks' offsets start at 0 again
    reads = case["reads"]
    pl = ec.plan(reads.start, reads.end, 1)
    st = ec.stream(case["tree"])
    assert len(st["pos"]) == 2 * n_mut
    block = np.arange(len(st["pos"])) // ec.SEL_EVENTS
    for g in range(pl["G"]):
        inside = (st["pos"] >= pl["group_ws"][g]) & (st["pos"] <= pl["group_we"][g])
        assert (block[inside] < ec.SEL_SCAN_WIDTH).any() and (block[inside] >= ec.SEL_SCAN_WIDTH).any()
    case["gen"].close()


# ---- D. list cap ----------------------------------------------------------------------------------------------------
def test_list_cap_case_sits_on_the_cap(oracle):
    case = ec.list_cap_case()
    tree, reads = case["tree"], case["reads"]
    n = tree.n_nodes
    want = oracle.OracleTree(tree).epp_map(reads, genome_size=case["genome"])
    assert (want["multiplicity"] == case["kind"]).all() and set(case["kind"].tolist()) == {1, 2, n}
    pl = ec.plan(reads.start, reads.end, 1)
    assert pl["ntiles"] == 1
    in_order = case["kind"][pl["order"]]
    assert (np.diff(in_order) != 0).sum() >= 20                      # the kinds are interleaved in window order
    assert case["caps"] == (0, 1, n - 1, n, n + 1)
    kept = [tuple(ec.cut_lists(want, cap)[1].tolist()) for cap in case["caps"]]
    assert sum(kept[0]) == 0 and sum(kept[1]) == 16 and sum(kept[2]) == 32 and sum(kept[3]) == 48
    assert len(set(kept[:4])) == 4 and kept[4] == kept[3]            # every cap up to n changes who keeps a list
    assert len(ec.cut_lists(want, n - 1)[0]["epp_nodes"]) == 16 * 1 + 16 * 2
    assert len(ec.cut_lists(want, n)[0]["epp_nodes"]) == 16 * (3 + n)


# ---- E. exact scores ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ec.SCORE_BATCHES)
@pytest.mark.parametrize("which", sorted(ec.DEGREE_TOTALS))
def test_score_batches_have_their_totals(oracle, which, batch):
    k = {"k52": 52, "k51": 51, "k31": 31}[which]
    case = ec.score_case(which, batch)
    reads, tree = case["reads"], case["tree"]
    total = int(reads.degree.astype(np.int64).sum())
    assert total == ec.DEGREE_TOTALS[which] and ec.fx_bits(total) == k and total < 2 ** 31
    assert (reads.degree >= 1).all() and (tree.mut_pos >= 0).all()
    if which == "k31":
        assert (reads.degree == 2 ** 28).sum() == 7 and (reads.degree <= 2).sum() >= reads.n_reads - 8
    want = oracle.OracleTree(tree).epp_map(reads, genome_size=case["genome"])
    exact, n_contrib, deg_sum = ec.exact_scores(want, reads.degree, tree.n_nodes)
    # the oracle's double sum lies within its own rounding of the exact one, and its counts are the degree sums
    for n in range(tree.n_nodes):
        assert abs(Fraction(float(want["score"][n])) - exact[n]) <= exact[n] * Fraction(int(n_contrib[n]) + 1, 2 ** 52)
    assert (want["counts"].astype(np.int64).sum(axis=1) == deg_sum).all()
    assert ((n_contrib == 0) == (want["score"] == 0)).all()
    # the bound holds for the arithmetic it was derived from ...
    over = lambda sc: [n for n in range(tree.n_nodes)
                       if abs(Fraction(float(sc[n])) - exact[n]) > ec.score_bound(exact[n], n_contrib[n], total)]
    assert not over(ec.fixed_point_scores(want, reads.degree, tree.n_nodes))
    if batch == "sparse":
        # ... and here it is tight enough to tell truncation from rounding to nearest (where every haplotype collects
        # dozens of reads the roundings average out below it), and some haplotypes collect nothing at all
        assert (want["multiplicity"][:len(ec.SPARSE_SIZES)] == ec.SPARSE_SIZES).all() and (n_contrib <= 8).all()
        assert len(over(ec.fixed_point_scores(want, reads.degree, tree.n_nodes, truncate=True))) >= 3
        assert (n_contrib == 0).any()
    else:
        assert (n_contrib > 50).any()


# ---- F. reads per lane, LDS limit -----------------------------------------------------------------------------------
def test_rpl_switch_cases_sit_on_the_switch():
    for longest, rpl, groups in ((383, 4, 2), (384, 1, 5)):
        case = ec.rpl_switch_case(longest)
        reads = case["reads"]
        assert reads.n_reads == 300 and int((reads.end - reads.start).max()) == longest
        assert ec.effective_rpl(reads.start, reads.end, 4) == rpl
        pl = ec.plan(reads.start, reads.end, rpl)
        assert pl["G"] == groups and pl["tile_reads"] == 64 * rpl
    assert ((383 >> 3) + 1) * 1024 == 48 * 1024 < ((384 >> 3) + 1) * 1024


def test_lds_limit_cases_sit_on_the_limit():
    below, above = ec.lds_limit_spans()
    assert above == below + 1
    assert ec.lds_bytes(below) <= 150 * 1024 < ec.lds_bytes(above)
    for span in (below, above):
        case = ec.lds_limit_case(span)
        reads = case["reads"]
        assert reads.n_reads == 1 and reads.end[0] - reads.start[0] == span and reads.end[0] <= case["genome"] == 6000
        pos = reads.read_word & 0xFFFFF
        assert pos.min() == reads.start[0] and pos.max() == reads.end[0] and len(pos) > 3      # both ends of the table are used
