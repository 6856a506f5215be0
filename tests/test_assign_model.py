"""The NumPy model of wepp_epp_assign (tests/assign_model.py) against the oracle's restatement of
haplotype::mutation_distance (OracleTree.epp_distance, src/WEPP/haplotype.hpp:123-173) and a literal restatement
of the read loop of arena::dump_read2haplotype_mapping (src/WEPP/arena.cpp:612-665); the argument errors of the
entry point that need no device."""
import ctypes

import numpy as np

import assign_model
import epp_fuzz
import fuzz_trees as ft
import wepp_amd as w
from wepp_amd import _lib


def reference_mapping(otree, reads, genome_size, sel):
    """arena.cpp:612-665, line by line, on OracleTree.epp_distance: epps per read in `abundance` (= sel) order,
    the reads of every haplotype, the count of :859-865 and the per-site coverage vectors."""
    K = len(sel)
    pos, ref, mut, _ = w.unpack_read_word(reads.read_word)
    min_dists, epp_sets = [], []
    hap_reads = [[] for _ in range(K)]
    hap_degree = [0] * K
    coverage = [[0] * genome_size for _ in range(K)]                       # :601-607
    for i in range(reads.n_reads):
        a, b = int(reads.read_off[i]), int(reads.read_off[i + 1])
        start, end = int(reads.start[i]), int(reads.end[i])
        dist = otree.epp_distance(pos[a:b], ref[a:b], mut[a:b], start, end)
        epps = []
        min_dist = 2**31 - 1
        for k in range(K):                                                 # :616-625
            curr_dist = int(dist[int(sel[k])])
            if curr_dist <= min_dist:
                if curr_dist < min_dist:
                    min_dist = curr_dist
                    epps.clear()
                epps.append(k)
        for k in epps:                                                     # :629-635
            hap_reads[k].append(i)
            hap_degree[k] += int(reads.degree[i])
        masked_sites = [int(p) for p, m in zip(pos[a:b], mut[a:b]) if m == 0b1111]   # :638-643
        update_sites = [j for j in range(start, end + 1) if j not in masked_sites]   # :645-650
        if update_sites:
            for k in epps:                                                 # :654-664
                for j in update_sites:
                    if j >= 1 and j <= genome_size:
                        coverage[k][j - 1] = 1
        min_dists.append(min_dist)
        epp_sets.append(epps)
    return min_dists, epp_sets, hap_reads, hap_degree, coverage


def odd_reads(rng, ref, genome, n_reads):
    """reads whose entries also lie outside their window, and windows that end past the genome (and past the
    tree's last mutated position)"""
    reads, start, end, degree = [], [], [], []
    for _ in range(n_reads):
        s = int(rng.integers(1, genome + 1))
        e = int(rng.integers(s, genome + 21))
        k = int(rng.integers(0, 9))
        ents = []
        for p in sorted(set(int(x) for x in rng.integers(1, genome + 16, size=k))):
            r = ref.get(p, 1)
            a = 15 if rng.random() < 0.25 else int(rng.integers(1, 15))
            if a == r:
                continue
            ents.append((p, r, a, 1 if a == 15 else 0))
        reads.append(ents)
        start.append(s); end.append(e); degree.append(int(rng.integers(0, 5)))
    return w.EppReads.from_lists(reads, start, end, degree)


def check_against_reference(oracle, tree, reads, genome, sel):
    got = assign_model.assign(tree, reads, genome, sel)
    ot = oracle.OracleTree(tree)
    min_dists, epp_sets, hap_reads, hap_degree, coverage = reference_mapping(ot, reads, genome, sel)
    ot.close()
    assert got["min_dist"].tolist() == min_dists
    assert got["n_epp"].tolist() == [len(x) for x in epp_sets]
    for r, epps in enumerate(epp_sets):
        assert got["asg_sel"][int(got["asg_off"][r]):int(got["asg_off"][r + 1])].tolist() == epps, r
    assert got["sel_reads"].tolist() == [len(x) for x in hap_reads]
    assert got["sel_degree"].tolist() == hap_degree
    assert got["sel_covered"].tolist() == [sum(c) for c in coverage]
    bits = np.unpackbits(got["cover_bits"].view(np.uint8), axis=1, bitorder="little")[:, :genome]
    assert np.array_equal(bits, np.array(coverage, np.uint8).reshape(len(sel), genome))


def test_model_matches_mutation_distance_and_the_reference_loop(oracle):
    rng = np.random.default_rng(20260)
    n_fuzz = n_odd = 0
    for it in range(60):
        genome = 60
        tree, ref = ft.random_tree(rng, genome=genome)
        n = tree.n_nodes
        K = int(rng.integers(1, n + 1))
        sel = rng.permutation(n)[:K].astype(np.uint32)
        reads = epp_fuzz.random_epp_reads(rng, tree, ref, genome, n_reads=30)
        check_against_reference(oracle, tree, reads, genome, sel)
        n_fuzz += reads.n_reads
        odd = odd_reads(rng, ref, genome, 20)
        # a genome that is no multiple of 32, and one shorter than some windows
        check_against_reference(oracle, tree, odd, int(rng.choice([genome, 45, 70])), sel)
        n_odd += odd.n_reads
    assert n_fuzz == 1800 and n_odd == 1200


def test_closed_form_on_every_haplotype(oracle):
    """the table's distances against epp_distance for ALL haplotypes of a tree (sel = identity)"""
    rng = np.random.default_rng(77)
    for it in range(10):
        tree, ref = ft.random_tree(rng, genome=60)
        ot = oracle.OracleTree(tree)
        tab = assign_model.SelectionTable(tree, np.arange(tree.n_nodes))
        for reads in (epp_fuzz.random_epp_reads(rng, tree, ref, 60, n_reads=20), odd_reads(rng, ref, 60, 20)):
            pos, rf, mut, _ = w.unpack_read_word(reads.read_word)
            for r in range(reads.n_reads):
                a, b = int(reads.read_off[r]), int(reads.read_off[r + 1])
                s, e = int(reads.start[r]), int(reads.end[r])
                assert np.array_equal(tab.distances(pos[a:b], mut[a:b], s, e), ot.epp_distance(pos[a:b], rf[a:b], mut[a:b], s, e))
        ot.close()


def _call(mat, rd, genome, n_sel, sel, out):
    return _lib.lib.wepp_epp_assign(mat, rd, genome, n_sel, sel, out)


def test_argument_errors_need_no_device():
    """null pointers, an empty selection and a repeated index are refused before the handle is looked at"""
    reads = w.EppReads.from_lists([[(3, w.A, w.C)]], [1], [10])
    rd = _lib.EppReadsC(1, reads.read_off.ctypes.data, reads.read_word.ctypes.data, reads.start.ctypes.data,
                        reads.end.ctypes.data, reads.degree.ctypes.data)
    out = _lib.AssignOutC()
    sel = np.array([2, 5, 2], np.uint32)
    selp = sel.ctypes.data_as(ctypes.c_void_p)
    err = lambda: _lib.lib.wepp_last_error().decode()
    assert _call(None, None, 60, 3, selp, ctypes.byref(out)) == 1 and "null argument" in err()
    assert _call(None, ctypes.byref(rd), 60, 3, selp, None) == 1 and "null argument" in err()
    assert _call(None, ctypes.byref(rd), 60, 3, None, ctypes.byref(out)) == 1 and "null argument" in err()
    assert _call(None, ctypes.byref(rd), 60, 0, selp, ctypes.byref(out)) == 1 and "empty selection" in err()
    assert _call(None, ctypes.byref(rd), 60, 3, selp, ctypes.byref(out)) == 1 and "selected more than once" in err()
    assert _call(None, ctypes.byref(rd), 60, 2, selp, ctypes.byref(out)) == 1 and "null argument" in err()   # no handle
    d = [ctypes.c_double(-1) for _ in range(3)]
    assert _lib.lib.wepp_epp_assign_last_timing(*[ctypes.byref(x) for x in d]) == 0
    assert w.epp_assign_last_timing() == dict(tables_ms=0.0, assign_ms=0.0, finish_ms=0.0)
