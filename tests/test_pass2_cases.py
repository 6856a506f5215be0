"""tests/pass2_cases.py held to its edges on the CPU: the restated chunk rule against hand-computed values, and for
every builder the fact about its INPUT that makes it an edge case -- chunk counts and lengths, checkpoint word counts,
events per block and the slots a read hits, the chunk of every tie, pair counts --, read from the flat image, the rule
and the oracle.  The per-node score cases also go through the Python model of the sweep (tests/sweep_model.py), cut
into the chunks the rule gives, against the oracle: the chunk-start arithmetic is held on the CPU as well."""
import numpy as np
import pytest

import pass2_cases as pc


_of_kind = pc.of_kind


# ---- the rule ----------------------------------------------------------------------------------------------------------
def test_constants_come_from_the_sources():
    assert (pc.BLK_MAX_NODES, pc.BLK_MAX_EVENTS, pc.TARGET_WAVES, pc.MIN_CHUNK_BLOCKS) == (64, 128, 8192, 8)


@pytest.mark.parametrize("n_reads, NB, ncp, cp_stride, scores, best", [
    # one read: a chunk per checkpoint; the list of optimal nodes takes NB / 8 chunks, one below 16 blocks
    (1, 7, 7, 1, (7, 1), (1, 7)),
    (1, 8, 8, 1, (8, 1), (1, 8)),
    (1, 16, 16, 1, (16, 1), (2, 8)),
    (1, 1024, 1024, 1, (1024, 1), (128, 8)),
    # 1025 blocks: a checkpoint every second block, 513 of them; 128 chunks wanted -> 5 checkpoints = 10 blocks each
    (1, 1025, 513, 2, (513, 2), (103, 10)),
    (3, 1025, 513, 2, (513, 2), (103, 10)),
    # ceil(8192 / n_reads) chunks wanted: 2, 1, 1
    (8191, 1024, 1024, 1, (2, 512), (2, 512)),
    (8192, 1024, 1024, 1, (1, 1024), (1, 1024)),
    (8193, 1024, 1024, 1, (1, 1024), (1, 1024)),
    (8191, 7, 7, 1, (2, 4), (1, 7)),
    (8191, 8, 8, 1, (2, 4), (1, 8)),
    (8191, 1025, 513, 2, (2, 514), (2, 514)),
    (8192, 1025, 513, 2, (1, 1026), (1, 1026)),
    # bpc rounds up, the chunk count follows from it: 82 wanted, 13 blocks each, 79 chunks, the last of 10 blocks
    (100, 1024, 1024, 1, (79, 13), (79, 13)),
    (4096, 7, 7, 1, (2, 4), (1, 7)),
    (4097, 7, 7, 1, (2, 4), (1, 7)),
    (4096, 33, 33, 1, (2, 17), (2, 17)),
])
def test_pass2_chunks_table(n_reads, NB, ncp, cp_stride, scores, best):
    assert pc.pass2_chunks(n_reads, NB, ncp, cp_stride, False) == scores
    assert pc.pass2_chunks(n_reads, NB, ncp, cp_stride, True) == best


def test_debug_line_parser():
    err = "[plan] x\n[scores] n_reads=3 nchunks=607 bpc=2\n[best_nodes] window 4: 17 reads nchunks=2 bpc=9\n[best_nodes] stream 11: 1 reads nchunks=1 bpc=3\n"
    assert pc.parse_debug_lines(err) == ([(3, 607, 2)], [("window", 4, 17, 2, 9), ("stream", 11, 1, 1, 3)])


def test_every_case_is_small():
    for name, fn in pc.CASES.items():
        c = fn()
        assert c.tree.n_nodes <= 20000, name
        for call in c.calls:
            b = call[0] if isinstance(call, tuple) else call
            assert b.n_reads <= pc.TARGET_WAVES, name


# ---- per-node scores -----------------------------------------------------------------------------------------------------
def test_chunk_rule_cases():
    c = pc.CASES["chunks_one"]()
    NB = c.geom()["NB"]
    assert NB == 2 and [b.n_reads for b in c.calls] == [8192, 8191]
    assert c.chunks(8192) == (1, NB) and c.chunks(8191) == (2, 1)
    c = pc.CASES["chunks_per_checkpoint"]()
    g = c.geom()
    assert g["cp_stride"] == 1 and g["NB"] >= 16 and all(b.n_reads == 1 and c.chunks(1) == (g["NB"], 1) for b in c.calls)
    assert c.calls[0].lists == [[]] and len(c.calls[1].lists[0]) >= 5 and all(e[3] == 1 for e in c.calls[1].lists[0])
    assert len(c.calls[2].lists[0]) >= 4
    c = pc.CASES["chunks_ragged"]()
    NB = c.geom()["NB"]
    (n1, b1), (n0, b0) = (c.chunks(b.n_reads) for b in c.calls)
    assert b1 >= 2 and NB % b1 == 1 and n1 == NB // b1 + 1          # a last chunk of exactly one block
    assert b0 >= 2 and NB % b0 == 0 and n0 == NB // b0 >= 2
    assert b1 != b0


def test_stride_2_case():
    c = pc.CASES["stride_2"]()
    g = c.geom()
    assert g["NB"] > 1024 and g["cp_stride"] >= 2 and g["ncp"] == -(-g["NB"] // g["cp_stride"]) and c.tree.n_nodes < 20000
    assert c.calls[0].n_reads == 3
    nchunks, bpc = c.chunks(3)
    assert (nchunks, bpc) == (g["ncp"], g["cp_stride"]) and g["NB"] % bpc != 0       # chunks start at multiples of two blocks, the last one is ragged
    # every read lists positions that are open at chunk starts with a non-zero enter_delta
    assert all(m >= 100 for m in c.facts["chunk_starts_moved"]), c.facts


def test_deep_checkpoint_cases():
    for i, counts in enumerate(([0, 64, 128, 192], [0, 65, 129, 193])):
        c = pc.CASES["deep_checkpoint_%d" % i]()
        flat = c.info.flat
        assert pc.cp_word_counts(flat).tolist() == counts and c.chunks(2) == (4, 1)
        l, short = c.calls[0].lists
        # the read's words among the checkpoint's: one per round of 64 lanes
        assert [x // pc.WAVE for x in pc.cp_hits(flat, l, 3)] == [0, 1, 2]
        assert [x // pc.WAVE for x in pc.cp_hits(flat, l, 2)] == [0, 1] and [x // pc.WAVE for x in pc.cp_hits(flat, l, 1)] == [0]
        assert [x // pc.WAVE for x in pc.cp_hits(flat, short, 3)] == [1, 2]         # (nothing in the first round)
        fm = pc.whole_tree_model(flat)
        assert fm.chunk_start_c(l, 3) == fm._c_none(l) - 2 * 3                      # each shared open mutation: -2


def test_block_edges_case():
    c = pc.CASES["block_edges"]()
    flat, who = c.info.flat, c.facts["who"]
    shape = pc.block_shape(flat)
    assert shape[0] == (64, 66, 1) and shape[1] == (64, 64, 0) and shape[2] == (64, 128, 0)      # 65 events and the padding one
    assert shape[3] == (3, pc.HEAVY + 2, 0) and shape[4] == (1, 2 * pc.HEAVY, 0) and 2 * pc.HEAVY > pc.BLK_MAX_EVENTS
    assert len(shape) == 7 and pc.HEAVY > 64
    assert int(flat.get("dfs2id")[int(flat.get("blk_node0")[4])]) == who["y"]
    special = c.calls[0].lists[0]
    hits = pc.event_hits(flat, special)
    by_block = {b: [h for h in hits if h[0] == b] for b in range(7)}
    assert (0, 1, 0, False, False) in by_block[0]                     # the root's own mutation: node offset 0 of block 0
    assert (0, 64, 63, False, True) in by_block[0]                    # offset 63, the second round, next to the padding event
    assert [h[1] // 64 for h in by_block[1]] == [0] and sorted(h[1] // 64 for h in by_block[2]) == [0, 1]
    assert by_block[3] == [(3, 3, 0, False, False)]                   # X's enter event ...
    assert (4, 3, 0, True, False) in by_block[4]                      # ... its exit in front of Y, the first round of Y's block
    assert (4, 2 * pc.HEAVY - 1, 0, False, False) in by_block[4]      # Y's last enter event: the third round, beyond event 128
    assert [h for h in by_block[5] if h[3]] == [(5, pc.HEAVY, 1, True, False)]   # Y's last exit in front of W, behind the leaf's event: later blocks inherit its net
    assert not by_block[6]
    # the running count at the start of blocks 3 .. 6: the root's mutation; X open; X closed and Y open; Y closed
    fm = pc.whole_tree_model(flat)
    trace = {}
    fm.place(special, node_scores=np.zeros(fm.N, np.int64), trace_c=trace)
    assert [trace[b] - fm._c_none(special) for b in (3, 4, 5, 6)] == [-2, -4, -4, -2]
    assert [c.chunks(b.n_reads) for b in c.calls] == [(7, 1), (7, 1), (2, 4), (1, 7)]


def test_eligibility_case():
    c = pc.CASES["eligibility"]()
    flat, lists = c.info.flat, c.calls[0].lists
    masked = pc.node_state(flat, lists[0], 9)
    assert masked["masked"] and masked["touched"] and masked["leaf"]
    assert pc.node_state(flat, lists[1], 2)["masked"] and pc.node_state(flat, lists[1], 2)["touched"]
    leaf_static, leaf = pc.node_state(flat, [], 5), pc.node_state(flat, lists[1], 5)
    assert leaf["leaf"] and leaf["touched"] and not leaf["masked"] and leaf_static["ncom"] == 1 and leaf["ncom"] == 0
    shared, unshared = pc.node_state(flat, lists[2], 6), pc.node_state(flat, lists[3], 6)
    assert not shared["leaf"] and shared["touched"] and shared["ncom"] == shared["nmut"] == 2
    assert unshared["touched"] and unshared["ncom"] == 0 < unshared["nmut"]
    # the node that does not compete reports one more than its set difference
    want = pc.want_scores("eligibility", 0)
    d2b = flat.get("dfs2bfs")
    d6 = int(np.flatnonzero(flat.get("dfs2id") == 6)[0])
    fm = pc.whole_tree_model(flat)
    assert want[3][d2b[d6]] == pc.model_scores(fm, lists[3], 1)[d6]


@pytest.mark.parametrize("name", _of_kind("scores"))
def test_model_of_the_sweep_cut_into_the_rule_s_chunks(oracle, name):
    c = pc.CASES[name]()
    flat = c.info.flat
    fm = pc.whole_tree_model(flat)
    d2b = flat.get("dfs2bfs")
    for i, b in enumerate(c.calls):
        nchunks, bpc = c.chunks(b.n_reads)
        want = pc.want_scores(name, i)
        assert want.shape == (len(b.lists), c.tree.n_nodes)
        for q, l in enumerate(b.lists):
            got = pc.model_scores(fm, l, bpc)
            assert (got == want[q][d2b]).all(), (name, i, q)


# ---- all optimal nodes ---------------------------------------------------------------------------------------------------
def test_ties_span_chunks_case():
    c = pc.CASES["ties_span_chunks"]()
    g = c.geom()
    nchunks, bpc = c.chunks(3)
    assert g["NB"] // pc.MIN_CHUNK_BLOCKS == nchunks == 5 < min(g["ncp"], pc.TARGET_WAVES // 3) and bpc == 10      # the NB / 8 cap decides
    assert c.chunks(1) == (nchunks, bpc)
    (s0, n0, t0), (s1, n1, t1), (s2, n2, t2) = pc.want_best("ties_span_chunks", 0)
    blk = pc.block_of_bfs(c.info.flat)
    assert n0 == len(t0) == pc.STAR_LEAVES > 1000
    per_chunk = np.bincount(blk[t0] // bpc, minlength=nchunks)
    assert len(per_chunk) == nchunks and per_chunk.min() > 100, per_chunk         # ties in every chunk: appends from every wave of the read
    assert n1 == 1 and blk[t1[0]] == g["NB"] - 1 and blk[t1[0]] // bpc == nchunks - 1 and g["NB"] % bpc != 0
    assert n2 == 1 and t2.tolist() == [0] and s2 == 0 and s0 == s1 == 0
    assert [crowns for _, crowns in c.calls] == [False, True, False]


def test_cap_and_one_chunk_cases():
    c = pc.CASES["nb_over_8"]()
    NB = c.geom()["NB"]
    assert NB < pc.MIN_CHUNK_BLOCKS and c.chunks(c.calls[0][0].n_reads) == (1, NB) and c.chunks(1, emit=False) == (NB, 1)
    c = pc.CASES["many_reads_few_ties"]()
    b = c.calls[0][0]
    assert b.n_reads == pc.TARGET_WAVES and c.chunks(b.n_reads) == (1, c.geom()["NB"]) and c.chunks(b.n_reads - 1)[0] == 2
    # with work skipping on the reads part into several tree-wide streams: every list a strict subset
    assert len(c.facts["routes"]) >= 3 and [crowns for _, crowns in c.calls] == [False, True]
    want = pc.want_best("many_reads_few_ties", 0)
    assert max(n for _, n, _ in want) < 200 and all(n == len(t) >= 1 for _, n, t in want)


def test_plans_mixed_case():
    c = pc.CASES["plans_mixed"]()
    f = c.facts
    last = c.info.flat.n_streams - 1
    assert last in f["routes"] and len(f["routes"]) >= 3           # tree-wide streams, the whole tree among them
    assert f["in_window"] >= 20 and f["window_crowns"] >= 10       # reads confined to a genome window whose stream is a crown
    assert f["whole_tree"] >= 5                                    # reads across windows, beyond every crown's bound
    assert [crowns for _, crowns in c.calls] == [True, False]


# ---- imputed and excess mutations ----------------------------------------------------------------------------------------
def test_pairs_256_case():
    c = pc.CASES["pairs_256"]()
    totals = []
    for b, bj in c.calls:
        per = [len(pc.ambiguous_entries(l)) for l in b.lists]
        totals.append(sum(per))
        assert len(bj) == b.n_reads and bj.max() < c.tree.n_nodes
        if sum(per):
            zero = [i for i, k in enumerate(per) if k == 0]
            assert zero[0] == 0 and zero[-1] == len(per) - 1 and any(0 < i < len(per) - 1 and per[i - 1] and per[i + 1] for i in zero)
            assert any(e[3] and e[2] == 15 for e in b.lists[0])            # (a missing N: more than one allele, no pair)
    assert totals == [pc.IMPUTED_THREADS - 1, pc.IMPUTED_THREADS, pc.IMPUTED_THREADS + 1, 0]


def test_pairs_128_case():
    c = pc.CASES["pairs_128"]()
    assert [len(pr) for _, pr, _ in c.calls[:3]] == [pc.EXCESS_THREADS - 1, pc.EXCESS_THREADS, pc.EXCESS_THREADS + 1]
    assert c.info.muts(0) == []
    for i, (b, pr, pj) in enumerate(c.calls[:3]):
        want = pc.want_excess("pairs_128", i)
        assert (pr[5], pj[5]) == (pr[4], pj[4]) and want[5] == want[4] and want[4]
        assert want[7] == [] and want[6] and want[8] and b.lists[pr[7]] == [] and pj[7] == 0
    assert all(x == [] for x in pc.want_excess("pairs_128", 3)) and len(c.calls[3][1]) == 3


def test_every_node_cases():
    ci, ce = pc.CASES["every_node_imputed"](), pc.CASES["every_node_excess"]()
    info = ci.info
    n = info.tree.n_nodes
    assert 50 <= n <= 70 and ci.tree is ce.tree
    # the tree: a root with mutations, masked nodes, position 10 forward - back (masked) - forward down one path
    assert len(info.muts(0)) == 2 and all(p > 0 for p, _, _, _ in info.muts(0))
    par = info.tree.parent.tolist()
    assert (par[3], par[2], par[1]) == (2, 1, 0)
    at10 = [[m for m in info.muts(x) if m[0] == 10][0] for x in (1, 2, 3)]
    r = pc.ref_of(10)
    assert at10[0][1:3] == (r, r) and at10[0][3] != r and at10[1][2:] == (at10[0][3], r) and at10[2][2] == r and at10[2][3] not in (r, at10[0][3])
    assert (-1, 0, 0, 0) in info.muts(2) and (-1, 0, 0, 0) in info.muts(9) and pc.node_state(info.flat, [], 2)["masked"]
    # the reads: node 6's own mutations at ambiguous entries, one shared and one not; positions nobody mutates
    lists = ci.calls[0][0].lists
    assert lists == ce.calls[0][0].lists
    first = {e[0]: e for e in lists[0]}
    m20, m21 = (next(m for m in info.muts(6) if m[0] == p) for p in (20, 21))
    assert first[20] in pc.ambiguous_entries(lists[0]) and first[20][2] & m20[3] and first[21] in pc.ambiguous_entries(lists[0]) and not first[21][2] & m21[3]
    assert 75 not in info.ref_at and 76 not in info.ref_at
    assert first[75][2] & first[75][1] and not first[76][2] & first[76][1] and first[76] in pc.ambiguous_entries(lists[0])
    assert [] in lists and sum(len(pc.ambiguous_entries(l)) for l in lists) >= 15
    # every (read, node) pair
    b, bj = ci.calls[0]
    assert sorted(zip(b.index.tolist(), bj.tolist())) == [(q, j) for q in range(len(lists)) for j in range(n)]
    _, pr, pj = ce.calls[0]
    assert sorted(zip(pr.tolist(), pj.tolist())) == [(q, j) for q in range(len(lists)) for j in range(n)]
    # the lowest-set-bit branch and the found-on-the-path branch both occur in the oracle's answers
    want = pc.want_imputed("every_node_imputed", 0)
    at76 = set(nuc for x in want for p, nuc in x if p == 76)
    assert at76 == {first[76][2] & -first[76][2]}
    assert len(set(nuc for x in want for p, nuc in x if p == 10)) >= 2
    assert sum(len(x) for x in pc.want_excess("every_node_excess", 0)) > 2000


def test_deep_chain_cases():
    for name, rising in (("deep_descending_excess", False), ("deep_rising_excess", True)):
        c = pc.CASES[name]()
        t = c.tree
        assert t.n_nodes == pc.DEEP and t.parent.tolist() == [-1] + list(range(pc.DEEP - 1))
        pos = [c.info.muts(d)[0][0] for d in range(pc.DEEP)]
        assert pos == [pc.DEEP_P + d if rising else pc.DEEP_P - d for d in range(pc.DEEP)]
        b, pr, pj = c.calls[0]
        assert not set(e[0] for l in b.lists for e in l) & set(pos) and pj.tolist() == [pc.DEEP - 1, 0, pc.DEEP // 2] * 2
        want = pc.want_excess(name, 0)
        # every mutation above the chosen node is listed as a back-mutation, by position; the root's own at the root
        for x, j in zip(want, pj.tolist()):
            back = [m for m in x if m[0] in pos]
            assert [m[0] for m in back] == sorted(pos[:max(j, 1)]) and all(m[3] == m[1] for m in back)
    c = pc.CASES["deep_descending_imputed"]()
    b, bj = c.calls[0]
    amb = pc.ambiguous_entries(b.lists[0])
    assert len(amb) == 1 and amb[0][0] == pc.DEEP_P == c.info.muts(0)[0][0] and bj.tolist() == [pc.DEEP - 1, 0, pc.DEEP // 2]
    assert sum(1 for p in c.tree.mut_pos.tolist() if p == pc.DEEP_P) == 1
    root_allele = c.info.muts(0)[0][3]
    assert amb[0][2] & root_allele
    assert pc.want_imputed("deep_descending_imputed", 0) == [[(pc.DEEP_P, root_allele)]] * 3
