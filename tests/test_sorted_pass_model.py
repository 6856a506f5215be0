"""The sorted pass of a read with more than 64 events (place_dev.hpp: sorted_build, sorted_query) on the CPU: its
sequential restatement (sorted_pass_model.py) gives, field by field, what the all-pairs definition gives -- on the
index entries of real streams and on hand-made lists with the ties a sort can get wrong."""
import numpy as np

import sorted_pass_model as spm
import walk_model as wm
import wepp_amd as w
from test_sorted_pass_gpu import draw_reads


def test_hand_made_lists():
    rng = np.random.default_rng(11)
    cases = spm.hand_made(rng)
    assert {len(e) for _, e in cases} == set(spm.EDGE_SIZES)
    for name, ents in cases:
        want = spm.all_pairs(ents)
        for N in {n for n in (128, 256) if n >= len(ents)}:
            spm.assert_same(spm.sorted_pass(ents, N), want, f"{name}, N={N}")
    # the shapes are what they claim to be
    by_name = dict(cases)
    assert len({n for n, _, _ in by_name["one node, E=256"]}) == 1
    assert len({e for _, e, _ in by_name["all ends equal, E=255"]}) == 1
    chain = by_name["node == end chains, E=193"]
    assert {n for n, _, _ in chain} & {e for _, e, _ in chain}
    assert all(e == n + 1 for n, e, _ in by_name["leaves only, E=129"])
    assert (0, 128) in {(n, e) for n, e, _ in by_name["the root entry, E=128"]}
    assert max(e for _, e, _ in by_name["keys at 2^25 - 1, E=65"]) == (1 << 25) - 1


def test_no_cut_behind_the_end_reads_as_none():
    """the one field that is not bit for bit the all-pairs value: see sorted_pass_model.canonical"""
    ents = [(3, 5, spm.pack(1, 0, 0)), (1, 9, spm.pack(-1, 0, 0))]
    got, want = spm.sorted_pass(ents), spm.all_pairs(ents)
    assert got[1][4] == spm.NONE and want[1][4] >= 0x80000000      # nothing behind node 9
    assert got[0][4] == want[0][4] == 2 * (9 - 5) - 1              # the end of the other entry cuts
    spm.assert_same(got, want)


def test_entries_of_real_streams():
    """the first 120 reads of the batch of test_sorted_pass_gpu.py (9 - 16 entries on a small tree with few positions) in
    the whole-tree stream: many events, and among the reads of 65 - 256 events nearly all with several entries on one
    node, a shared subtree end and an entry node at another entry's end"""
    g = w.generate_tree(61, 6000, genome_len=400, p_ambiguous=0.02, p_masked_node=0.003, root_mutations=1)
    fv = w.FlatView(g.tree)
    model = wm.WalkModel(fv)
    samples, totals = draw_reads(g.tree, 3, 400)
    sizes, ties = [], [0, 0, 0]
    for S, total in list(zip(samples, totals))[:120]:
        ents = spm.entries_of(model, S)
        assert len(ents) == total
        if len(ents) > spm.MAX_EVENTS:
            continue
        sizes.append(len(ents))
        nodes, ends = [n for n, _, _ in ents], [e for _, e, _ in ents]
        if len(ents) > 64:
            ties[0] += len(set(nodes)) < len(nodes)
            ties[1] += len(set(ends)) < len(ends)
            ties[2] += bool(set(nodes) & set(ends))
        spm.assert_same(spm.sorted_pass(ents, 128 if len(ents) <= 128 else 256), spm.all_pairs(ents), f"E={len(ents)}")
    big = sum(s > 64 for s in sizes)
    print(len(sizes), big, sum(s > 128 for s in sizes), ties)
    assert big >= 80 and sum(s > 128 for s in sizes) >= 60, sizes
    # (of the whole batch's 326 such reads about five in six hold several entries on a node, nearly all the other two ties)
    assert ties[0] >= 0.7 * big and ties[1] >= 0.9 * big and ties[2] >= 0.9 * big, (ties, big)
    fv.close()
    g.close()
