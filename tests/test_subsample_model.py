"""The model of read subsampling (tests/subsample_model.py) against hand-computed values and its own definition, and
the condition every GPU case of tests/subsample_cases.py has to meet: every trial whose table differs from the winner's
exceeds the winner's divergence by more than the sum of the two rounding bounds -- a condition on the INPUTS (a case
that misses it gets another seed, never a wider margin).  The cases also have to show the edge they are named after."""
import math

import numpy as np
import pytest

import sam_model as sm
import subsample_cases as sc
import subsample_model as sub


def test_hash_vectors():
    """splitmix64 by hand: f(0) finalises the golden-ratio increment; the published stream of seed 0 is f(0), f(g), f(2g)"""
    g = 0x9E3779B97F4A7C15
    assert sub.f(0) == 0xE220A8397B1DCDAF
    assert sub.f(g) == 0x6E789E6AA1B965F4 and sub.f(2 * g & sub.MASK) == 0x06C45D188009454F
    assert sub.f(sub.MASK) == sub.f(-1 & sub.MASK) and 0 <= sub.f(sub.MASK) <= sub.MASK
    # key(t, r) = f(f(seed ^ f(t)) ^ r), spelled out
    seed, t, r = 0x0123456789ABCDEF, 5, 77
    assert sub.key(seed, t, r) == sub.f(sub.f(seed ^ sub.f(t)) ^ r)
    assert sub.key(0, 0, 0) == sub.f(sub.f(sub.f(0)))
    # the vectorised keys are the same function
    assert sub.keys(seed, t, 200).tolist() == [sub.key(seed, t, i) for i in range(200)]
    assert len(set(sub.keys(seed, t, 5000).tolist())) == 5000           # f is a bijection: no two keys of a trial are equal


@pytest.mark.parametrize("n,m", [(130, 1), (130, 64), (130, 129), (300, 257)])
def test_subsets(n, m):
    seed = 99
    for t in (0, 1, 17):
        k = sub.keys(seed, t, n)
        thr = sub.threshold(seed, t, n, m)
        assert thr == sorted(k.tolist())[m - 1]                          # the m-th smallest key
        members = sub.subset(seed, t, n, m)
        assert len(members) == m and members == sorted(members)
        assert set(members) == set(np.argsort(k)[:m].tolist())
    # a trial's subset depends on (seed, t, n, m) alone: the whole call with 3 and with 20 trials agrees on trials 0 .. 2
    ref, reads = sm.gen_aligned(1, G=200, n_reads=n)
    a = sub.subsample(ref, reads, sc.AF, 3, seed, m, 3)
    b = sub.subsample(ref, reads, sc.AF, 3, seed, m, 20)
    assert a["threshold"] == b["threshold"][:3] and a["divergence"] == b["divergence"][:3]
    assert all(np.array_equal(x, y) for x, y in zip(a["tables"], b["tables"]))


def test_tables_and_divergence_by_hand():
    """two sites: F = A:3 C:1 | G:2 (and an N the full table does not count); the subset holds A, A, N-at-site-2"""
    F = np.array([[3, 1, 0, 0, 0, 0], [0, 0, 2, 0, 0, 0]])
    A = np.array([[2, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0]])
    d, bound = sub.divergence(F, A)
    p = [3 / 8, 1 / 8, 2 / 4]
    q = [2 / 4, 1e-10, 1e-10]                                            # site 2 is covered by an N only: C_t = 2, q = 0 -> floor
    assert d == pytest.approx(sum(x * (math.log(x) - math.log(y)) for x, y in zip(p, q)), rel=1e-15)
    assert 0 < bound < 1e-12
    ref = "ACGTACGT"
    reads = [("a", 0, "AN"), ("b", 0, "A"), ("c", 0, "C"), ("d", 0, "AG"), ("e", 1, "G")]
    assert sm.frequency_table(reads, 8)[:2] == F.tolist()
    got = sub.trial_table(reads, 8, np.array([True, True, False, False, False]))
    assert got[:2].tolist() == A.tolist() and not got[2:].any()


def test_no_draw():
    ref, reads = sm.gen_aligned(2, G=200, n_reads=130)
    for m in (130, 131, 1000):
        got, want = sub.subsample(ref, reads, sc.AF, 3, 5, m, 7), sm.build(ref, reads, sc.AF, 3)
        assert got["best_trial"] is None and got["kept"] == list(range(130)) and got["divergence"] == [0.0] * 7
        assert all(got[k] == want[k] for k in want)


def test_winner_and_correction_under_the_full_table():
    ref, reads, min_af, min_depth, seed, m, T = sc.CASES["full_table"]
    got = sc.model("full_table")
    assert got["best_trial"] == min(range(T), key=lambda t: (got["divergence"][t], t))
    assert got["freq"] == sm.frequency_table(reads, len(ref))
    alone = sm.build(ref, [reads[i] for i in got["kept"]], min_af, min_depth)
    assert [c[2] for c in alone["corrected"]] != [c[2] for c in got["corrected"]], "the kept reads alone correct the same way"
    assert max(sum(row) for row in got["freq"]) >= min_depth > max(sum(row[:4]) + row[5] for row in got["tables"][got["best_trial"]].tolist())


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case_is_separated(name):
    m = sc.model(name)
    slack = sub.separated(m)
    assert slack is None or slack > 0, (name, slack)
    assert slack is not None or name in ("ties", "T1"), "every trial has the winner's table"


def test_cases_show_their_edges():
    m = sc.model("ties")
    assert len(set(m["divergence"])) == 1 and m["best_trial"] == 0
    m = sc.model("deep")
    assert m["tables"][m["best_trial"]].max() > 65535
    ref, reads = sc.CASES["floors"][:2]
    m = sc.model("floors")
    A, F = m["tables"][m["best_trial"]], np.array(m["freq"])
    assert ((F.sum(axis=1) > 0) & (A.sum(axis=1) == 0)).any(), "no site of the full table is left uncovered"
    assert (A[40, 4] == A[40].sum()) and A[40, 4] > 0 and F[40].sum() > 0, "site 41 is not covered by N alone"
    assert any(set(reads[i][2]) <= {"N", "_"} and "_" in reads[i][2] for i in m["kept"]), "no read of N and _ only is kept"
    for G in (sc.TILE - 1, sc.TILE, sc.TILE + 1, 2 * sc.TILE + 5):
        reads = sc.CASES[f"G{G}"][1]
        assert any(r[1] + len(r[2]) == G for r in reads) and any(r[1] == 0 for r in reads)
        for b in range(sc.TILE, G, sc.TILE):
            assert any(r[1] < b < r[1] + len(r[2]) for r in reads) and any(r[1] + len(r[2]) == b for r in reads) and any(r[1] == b for r in reads)
