"""tests/clades_model.py against the oracle (has_unique of the best node) and the id numbering wepp_mat_set_clades asks
for against the string sort of the reference (usher_common.cpp:614).  CPU only."""
import numpy as np
import pytest

import clades_model as cm
from fuzz_trees import random_sample, random_tree
from oracle_bridge import OracleTree
from wepp_amd import Tree, number_clade_names


def _place(ot, sample):
    pos = [e[0] for e in sample]; ref = [e[1] for e in sample]; mut = [e[2] for e in sample]; miss = [e[3] for e in sample]
    return ot.place_sample(pos, ref, mut, miss, want_best_vec=True)


def test_has_unique_of_best_node_matches_oracle():
    rng = np.random.default_rng(20261)
    seen = {0: 0, 1: 0}
    root_best = {True: 0, False: 0}      # the root as best node, with / without mutations of its own
    for t in range(120):
        tree, ref = random_tree(rng, root_muts=bool(t % 2))
        parent, muts = cm.tree_lists(tree)
        bfs, _kids = cm.bfs_order(parent)
        ot = OracleTree(tree)
        for _ in range(12):
            sample = random_sample(rng, ref)
            want = _place(ot, sample)
            node = bfs[want["best_j"]]
            assert node == want["best_node_id"]
            got = cm.has_unique(muts[node], parent[node] < 0, sample)
            assert int(got) == want["has_unique"], (t, sample, node)
            seen[int(got)] += 1
            if parent[node] < 0:
                root_best[bool([m for m in muts[node] if m[0] >= 0])] += 1
        ot.close()
    assert seen[0] > 50 and seen[1] > 50
    assert root_best[True] > 0 and root_best[False] > 0


def test_root_is_never_unique_whatever_it_carries():
    # a single-node tree: the root is the only candidate, with and without mutations (usher_mapper.cpp:191, :266-271)
    for root_muts in ([], [(5, 1, 1, 2), (9, 4, 4, 8)], [(-1, 0, 0, 0), (5, 1, 1, 2)]):
        tree = Tree.from_lists([-1], [root_muts])
        ot = OracleTree(tree)
        for sample in ([], [(5, 1, 2, 0)], [(5, 1, 4, 0), (7, 2, 15, 1)]):
            want = _place(ot, sample)
            assert want["best_j"] == 0 and want["has_unique"] == 0
            assert cm.has_unique(root_muts, True, sample) is False
        ot.close()


@pytest.mark.parametrize("column", [
    ["B.1", "", "A", "UNDEFINED", "Z", ""],                 # the reserved name is itself an annotation
    ["V", "A", "", "", "a", "U"],                           # UNDEFINED falls between other names (U < UNDEFINED < V < a)
    ["B.1", "B.1.1", "B", "B.1.1.7", "", "B.10"],           # a name is a prefix of another
    ["", "", "", "", "", ""],                               # nothing but UNDEFINED
    ["20A", "20A ", " 20A", "19B", "2", "20A/x"],           # bytes below and above the alphabet
])
def test_rank_numbering_reproduces_the_string_sort(column):
    cid, und, names = number_clade_names([column])
    ids = {nm: i + 1 for i, nm in enumerate(names[0])}
    assert ids["UNDEFINED"] == int(und[0])
    assert [int(x) for x in cid[0]] == [ids[a] if a else 0 for a in column]
    pool = [a for a in column if a] + ["UNDEFINED"]
    rng = np.random.default_rng(7)
    for _ in range(50):
        draw = [pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 40)))]
        by_name = sorted(draw)
        by_id = [names[0][i - 1] for i in sorted(ids[a] for a in draw)]
        assert by_id == by_name


def test_undefined_between_and_prefix_orders():
    _, und, names = number_clade_names([["V", "A", "", "a", "U"]])
    assert names[0] == ["A", "U", "UNDEFINED", "V", "a"] and int(und[0]) == 3
    _, _, names = number_clade_names([["B.1.1.7", "B.1", "B", "B.1.1", "B.10"]])
    assert names[0] == ["B", "B.1", "B.1.1", "B.1.1.7", "B.10", "UNDEFINED"]


def test_clade_assignment_walk():
    #      0 (R)
    #     / \
    #    1   2 (X)
    #   / \   \
    #  3   4   5 (Y)
    parent = [-1, 0, 0, 1, 1, 2]
    col = ["R", "", "X", "", "", "Y"]
    assert cm.clade_assignment(parent, col, 3, True) == "R"
    assert cm.clade_assignment(parent, col, 5, True) == "Y"
    assert cm.clade_assignment(parent, col, 5, False) == "X"
    assert cm.clade_assignment(parent, col, 0, True) == "R"
    assert cm.clade_assignment(parent, col, 0, False) == "UNDEFINED"
    assert cm.clade_assignment(parent, ["", "", "", "", "", ""], 4, True) == "UNDEFINED"
    assert cm.run_lengths(["A", "A", "B", "C", "C", "C"]) == [("A", 2), ("B", 1), ("C", 3)]
    assert cm.format_clades_row("s", [("B", ["A", "B", "B"]), ("U", ["U"])], True) == "s\tB*|A(1/3),B(2/3)\tU*|U(1/1)\n"
    assert cm.format_clades_row("s", [("B", ["A", "B", "B"]), ("U", ["U"])], False) == "s\tB\tU\n"
