"""The model of wepp_epp_resolve (tests/resolve_model.py: arena.cpp:746-892 line by line on the model table of
wepp_epp_assign) against a second formulation -- the oracle's haplotype::mutation_distance
(OracleTree.epp_distance) on the model's modified reads, minimum and ties in NumPy --, the hand cases of the
three-way rule spelt out, and the argument errors of the entry point that need no device."""
import ctypes

import numpy as np

import assign_model
import epp_fuzz
import fuzz_trees as ft
import resolve_cases as rc
import resolve_model as rm
import wepp_amd as w
from test_assign_model import odd_reads
from wepp_amd import _lib


def second_formulation(otree, modified, covered, masked, sel, K):
    """hap_reads / hap_degree from the oracle's distances of the modified reads, without the model's loop"""
    D = assign_model.oracle_distances(otree, modified)[:, np.asarray(sel, np.int64)]
    tie = D == D.min(axis=1, keepdims=True) if modified.n_reads else np.zeros((0, K), bool)
    M = len(covered)
    hr = np.zeros((M, K), np.uint32); hd = np.zeros((M, K), np.int64)
    for m in range(M):
        rows = np.array(sorted(covered[m] + masked[m]), np.int64)
        if rows.size:
            hr[m] = tie[rows].sum(axis=0)
            hd[m] = (tie[rows] * modified.degree[rows].astype(np.int64)[:, None]).sum(axis=0)
    return hr, hd


def test_model_matches_the_oracle_on_the_modified_reads(oracle):
    rng = np.random.default_rng(4242)
    total = dict.fromkeys(rm.BRANCHES, 0)
    n_repeated = ref_first = ref_second = 0
    for it in range(40):
        genome = 60
        tree, ref = ft.random_tree(rng, genome=genome)
        n = tree.n_nodes
        K = int(rng.integers(1, n + 1))
        sel = rng.permutation(n)[:K].astype(np.uint32)
        ot = oracle.OracleTree(tree)
        for reads in (epp_fuzz.random_epp_reads(rng, tree, ref, genome, n_reads=25), odd_reads(rng, ref, genome, 15)):
            residual = rc.draw_residual(rng, reads, ref, genome, int(rng.integers(1, 13)))
            rep, a, b = rc.repeated_positions(residual)
            n_repeated += len(rep); ref_first += a; ref_second += b
            got = rm.resolve(tree, reads, genome, sel, residual)
            for k, v in got["branches"].items():
                total[k] += v
            modified, covered, masked, _ = rm.mask_reads(reads, residual)
            hr, hd = second_formulation(ot, modified, covered, masked, sel, K)
            assert np.array_equal(got["hap_reads"], hr) and np.array_equal(got["hap_degree"], hd), it
            # best from the sums, the "appeared" rule in NumPy
            for m in range(len(residual)):
                app = hr[m] > 0
                mx = int(hd[m][app].max()) if app.any() else 0
                assert int(got["best_degree"][m]) == mx
                assert np.array_equal(got["best"][m], np.flatnonzero(app & (hd[m] == mx)))
        ot.close()
    assert all(v > 0 for v in total.values()), total
    assert n_repeated > 0 and ref_first > 0 and ref_second > 0


def _case(name):
    for c in rc.hand_cases():
        if c[0] == name:
            return c
    raise KeyError(name)


def _run(name):
    _, tree, reads, genome, sel, residual = _case(name)
    return rm.resolve(tree, reads, genome, sel, residual), reads


def _rel(out, m):
    a, b = int(out["rel_off"][m]), int(out["rel_off"][m + 1])
    return [(int(x) & 0x7FFFFFFF, "masked" if int(x) >> 31 else "covered") for x in out["rel_read"][a:b]]


def test_two_alleles_at_one_position_both_orders():
    # reads: 0 entry C at 10, 1 N at 10, 2 nothing at 10, 3 entry T at 10
    out, _ = _run("same-pos C,T/sel=[0, 1, 2, 3]")
    assert _rel(out, 0) == [(0, "covered"), (1, "masked")]                    # C: the entry becomes N
    assert _rel(out, 1) == [(0, "masked"), (1, "masked"), (3, "covered")]     # T: read 0's entry is N by now
    out, _ = _run("same-pos T,C/sel=[0, 1, 2, 3]")
    assert _rel(out, 0) == [(1, "masked"), (3, "covered")]                    # T first: read 0 still says C
    assert _rel(out, 1) == [(0, "covered"), (1, "masked"), (3, "masked")]
    out, _ = _run("same-pos ref,C/sel=[0, 1, 2, 3]")
    assert _rel(out, 0) == [(1, "masked"), (2, "covered")]                    # the reference allele: inserted into read 2
    assert _rel(out, 1) == [(0, "covered"), (1, "masked"), (2, "masked")]     # and masks it for the next one
    out, _ = _run("same-pos C,ref/sel=[0, 1, 2, 3]")
    assert _rel(out, 1) == [(0, "masked"), (1, "masked"), (2, "covered")]
    assert out["n_touched"] == 3


def test_insertions_keep_the_entries_sorted():
    out, reads = _run("insert/sel=[0, 1, 2, 3]")
    mod = out["modified"]
    for r in range(reads.n_reads):
        p = mod.entries(r)[0]
        assert np.all(np.diff(p) > 0)
    assert mod.entries(0)[0].tolist() == [4, 15, 20, 25, 30, 35, 40]          # before, between, after
    assert mod.entries(1)[0].tolist() == [15, 25, 35, 40]                     # into a read with no entries
    assert mod.entries(2)[0].tolist() == [4, 5, 15, 20, 25, 35, 40]
    assert _rel(out, 5) == [(0, "covered")]                                   # 20C: read 2 says G there


def test_window_bounds_are_inclusive():
    out, _ = _run("window/sel=[0, 1, 2, 3]")
    assert _rel(out, 0) == [(0, "covered")]           # pos == start of reads 0 and 1 (read 1 holds another allele), start - 1 of read 2
    assert _rel(out, 1) == [(0, "covered"), (1, "covered")]     # pos == end
    assert _rel(out, 2) == [] and _rel(out, 3) == []  # start - 1, end + 1
    assert _rel(out, 4) == [(0, "masked"), (1, "covered")]
    assert _rel(out, 5) == [(0, "masked"), (1, "masked"), (2, "covered")]


def test_beyond_the_trees_last_position_and_a_mutation_without_reads():
    out, _ = _run("beyond/sel=[0, 1, 2, 3]")
    assert _rel(out, 0) == [(0, "covered"), (2, "covered")]
    assert _rel(out, 1) == [(0, "masked"), (1, "covered"), (2, "masked")]
    assert _rel(out, 2) == [(2, "masked")]
    assert _rel(out, 3) == [(1, "covered"), (2, "covered")]       # 60: inside the window that ends at 70, outside the one that ends at 58
    for m in (4, 5):                                              # no read meets them
        assert _rel(out, m) == [] and int(out["best_degree"][m]) == 0 and out["best"][m].size == 0
        assert not out["hap_reads"][m].any() and not out["best_mask"][m].any()


def test_all_degree_zero_lists_the_haplotypes_that_appeared():
    out, _ = _run("degree 0/sel=[0, 1, 2, 3]")
    # 40T is carried by read 1 only (degree 0); with 40 masked the read (5C) is nearest to haplotypes 1 and 2
    assert _rel(out, 0) == [(1, "covered")]
    assert int(out["best_degree"][0]) == 0
    assert out["best"][0].tolist() == [1, 2]
    assert np.array_equal(out["best"][0], np.flatnonzero(out["hap_reads"][0] > 0))
    # the reference base at 20: reads 0, 1 (degree 0) and 2 (degree 7), all nearest to haplotype 1
    assert int(out["best_degree"][1]) == 7 and out["best"][1].tolist() == [1]
    assert out["hap_reads"][1].tolist() == [0, 3, 1, 0]


def test_tally_beyond_32_bits():
    out, _ = _run("int64/sel=[0, 1, 2, 3]")
    assert int(out["best_degree"][0]) == 3 * (2**31 - 1) > 2**32
    assert int(out["best_degree"][1]) == 4 * (2**31 - 1)
    assert out["hap_degree"].dtype == np.int64


def test_no_touched_read():
    out, _ = _run("untouched/sel=[0, 1, 2, 3]")
    assert out["n_touched"] == 0 and not out["rel_off"].any() and out["rel_read"].size == 0
    assert not out["best_mask"].any() and not out["best_degree"].any()


def test_argument_errors_need_no_device():
    """the checks shared with wepp_epp_assign answer with its codes and messages before the handle is looked at"""
    reads = w.EppReads.from_lists([[(3, w.A, w.C)]], [1], [10])
    rd = _lib.EppReadsC(1, reads.read_off.ctypes.data, reads.read_word.ctypes.data, reads.start.ctypes.data,
                        reads.end.ctypes.data, reads.degree.ctypes.data)
    out = _lib.ResolveOutC()
    sel = np.array([2, 5, 2], np.uint32)
    selp = sel.ctypes.data_as(ctypes.c_void_p)
    res = np.array([int(w.pack_read_word(3, w.A, w.C))], np.uint32)
    resp = res.ctypes.data_as(ctypes.c_void_p)
    call = lambda rdp, n_sel, s, n_res, r, o: _lib.lib.wepp_epp_resolve(None, rdp, 60, n_sel, s, n_res, r, o)
    err = lambda: _lib.lib.wepp_last_error().decode()
    assert call(None, 3, selp, 1, resp, ctypes.byref(out)) == 1 and "null argument" in err()
    assert call(ctypes.byref(rd), 3, selp, 1, resp, None) == 1 and "null argument" in err()
    assert call(ctypes.byref(rd), 0, selp, 1, resp, ctypes.byref(out)) == 1 and "empty selection" in err()
    assert call(ctypes.byref(rd), 3, selp, 1, resp, ctypes.byref(out)) == 1 and "selected more than once" in err()
    assert call(ctypes.byref(rd), 2, selp, 1, None, ctypes.byref(out)) == 1 and "null argument" in err()
    assert call(ctypes.byref(rd), 2, selp, 1, resp, ctypes.byref(out)) == 1 and "null argument" in err()   # no handle
    assert w.epp_resolve_last_timing() == dict(mark_ms=0.0, tables_ms=0.0, assign_ms=0.0, tally_ms=0.0)
