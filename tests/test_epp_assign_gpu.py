"""wepp_epp_assign on the GPU against the NumPy model of its kernels (tests/assign_model.py), the oracle's
haplotype::mutation_distance (OracleTree.epp_distance) and wepp_epp_map.  Everything is integer: bit-exact.

Layout units of k_assign whose two sides are covered below (assign.hpp): 4 haplotypes per lane, 256 per wave and
row load (a slab), 4 slabs = 1024 haplotypes whose distances stay in registers, 5120 columns up to which a
workgroup gathers its per-haplotype counts in LDS, 127 window entries between two flushes of the byte counters."""
import ctypes

import numpy as np
import pytest

import assign_model as am
import epp_fuzz
import fuzz_trees as ft
import wepp_amd as w
from wepp_amd import _lib

pytestmark = pytest.mark.gpu

GENOME = 29903


def _pick(rng, n, K):
    return rng.permutation(n)[:K].astype(np.uint32)


def test_fuzz_small_trees():
    rng = np.random.default_rng(90210)
    for it in range(40):
        genome = 60
        tree, ref = ft.random_tree(rng, genome=genome)
        reads = epp_fuzz.random_epp_reads(rng, tree, ref, genome, n_reads=int(rng.integers(1, 601)))
        n = tree.n_nodes
        K = min(n, [1, 2, 3, 4, 5, 63, 64, 65, n][it % 9])
        sel = _pick(rng, n, K)
        mat = w.Mat(tree)
        got = mat.epp_assign(reads, genome, sel, want_bits=True)
        am.check_equal(got, am.assign(tree, reads, genome, sel), (it, K))
        mat.close()


@pytest.fixture(scope="module")
def layout_case(oracle):
    """tree, reads and the oracle's [reads, haplotypes] distances, computed once per tree size"""
    cache = {}

    def get(n_nodes, n_reads):
        if n_nodes not in cache:
            g = w.generate_tree(11, n_nodes)
            reads = g.reads(12, n_reads, read_len=150, p_substitution=0.003, p_n=0.01, windows=True, max_degree=5)
            ot = oracle.OracleTree(g.tree)
            cache[n_nodes] = (g, reads, am.oracle_distances(ot, reads), w.Mat(g.tree))
            ot.close()
        return cache[n_nodes]
    yield get
    for g, _, _, mat in cache.values():
        mat.close()


@pytest.mark.parametrize("n_nodes,n_reads,K", [(600, 300, k) for k in (255, 256, 257, 511, 513)] +
                         [(1100, 300, k) for k in (1023, 1024, 1025)] + [(5200, 120, k) for k in (5120, 5121)])
def test_layout_edges(layout_case, n_nodes, n_reads, K):
    g, reads, D, mat = layout_case(n_nodes, n_reads)
    sel = _pick(np.random.default_rng(K), g.tree.n_nodes, K)
    want = am.assign_from_distances(lambda r: D[r, sel], K, reads, GENOME)
    got = mat.epp_assign(reads, GENOME, sel, want_bits=True)
    am.check_equal(got, want, K)
    t = w.epp_assign_last_timing()
    assert t["assign_ms"] > 0 and t["tables_ms"] > 0


def test_whole_tree_as_selection_equals_the_map():
    """no masked mutations: the reference's two formulations of the distance agree, so the map's parsimony,
    multiplicity and EPP lists are the assignment's; about 2 600 of 3 000 haplotypes tie per read"""
    g = w.generate_tree(5, 3000)
    reads = g.reads(6, 700, read_len=150, p_substitution=0.003, p_n=0.01, windows=True, max_degree=7)
    N = g.tree.n_nodes
    mat = w.Mat(g.tree)
    m = mat.epp_map(reads, GENOME, max_cached_epp=N, want_counts=False, want_divergence=False)
    got = mat.epp_assign(reads, GENOME, np.arange(N, dtype=np.uint32), want_bits=True)
    assert np.array_equal(got["min_dist"], m["max_parsimony"])
    assert np.array_equal(got["n_epp"], m["multiplicity"])
    assert np.array_equal(got["asg_off"], m["epp_off"]) and np.array_equal(got["asg_sel"], m["epp_nodes"])
    assert int(got["asg_off"][-1]) > 1000 * reads.n_reads
    # the per-haplotype outputs follow from the lists
    off, lst = m["epp_off"], m["epp_nodes"]
    best = m["max_parsimony"]
    dist = lambda r: np.where(np.isin(np.arange(N), lst[int(off[r]):int(off[r + 1])]), best[r], best[r] + 1)
    am.check_equal(got, am.assign_from_distances(dist, N, reads, GENOME), "whole tree")
    mat.close()


@pytest.mark.parametrize("genome", [GENOME, 60])
def test_coverage_edges(genome):
    # positions 5 and 40 mutated: haplotype 1 carries A5C, haplotype 2 adds G40T, 3 takes 5 back
    tree = w.Tree.from_lists([-1, 0, 1, 1], [[], [(5, w.A, w.A, w.C)], [(40, w.G, w.G, w.T)], [(5, w.A, w.C, w.A)]])
    Nn = (w.A, w.N, 1)
    reads, start, end, degree = [], [], [], []

    def add(ents, s, e, d=1):
        reads.append(ents); start.append(s); end.append(e); degree.append(d)
    for m in (1, 2):                                       # windows that start / end next to a word boundary
        for x in (32 * m - 1, 32 * m, 32 * m + 1):
            if x <= genome:
                add([], x, x)
                add([], 1, x)
                add([], x, min(genome, x + 40))
    add([], 36, 44)                                        # inside one word
    add([(40, w.G, w.T)], 34, 62, 3)
    add([], max(1, genome - 10), genome + 30)              # end > genome_size
    add([], genome, genome + 1)
    add([(10,) + Nn, (20,) + Nn], 10, 20, 2)               # N at the first and the last base of the window
    add([(p,) + Nn for p in range(50, 55)], 50, 54, 4)     # all N: counted, covers nothing
    add([(5, w.A, w.C)], 3, 9, 0)                          # degree 0
    add([(5, w.A, w.C)], 1, 30, 2)                         # two reads whose windows overlap on one haplotype:
    add([(5, w.A, w.C)], 20, 58, 2)                        # union, not sum
    add([(32,) + Nn, (33,) + Nn], 31, 34)                  # N on both sides of a word boundary
    rd = w.EppReads.from_lists(reads, start, end, degree)
    mat = w.Mat(tree)
    for sel in ([0, 1, 2, 3], [3, 1], [2]):
        got = mat.epp_assign(rd, genome, sel, want_bits=True)
        want = am.assign(tree, rd, genome, sel)
        am.check_equal(got, want, (genome, sel))
        pop = np.unpackbits(got["cover_bits"].view(np.uint8), axis=1).sum(axis=1)
        assert np.array_equal(pop, got["sel_covered"])
        assert (got["sel_covered"] <= genome).all() and got["sel_covered"].max() > 0
    # the all-N read is assigned (every haplotype ties at 0) and adds its degree
    full = mat.epp_assign(rd, genome, [0, 1, 2, 3])
    alln = len(reads) - 5
    assert full["n_epp"][alln] == 4 and full["min_dist"][alln] == 0
    mat.close()


@pytest.mark.parametrize("p_n,n_reads", [(0.05, 100), (0.2, 30)])
def test_long_reads(oracle, p_n, n_reads):
    """1 200 bp: more than 64 entries per read at 5 % N, more than 127 inside the window at 20 %"""
    g = w.generate_tree(5, 8000)
    reads = g.reads(21, n_reads, read_len=1200, amplicon_len=1200, amplicon_step=1000, p_substitution=0.003, p_n=p_n,
                    windows=True, max_degree=3)
    assert int(np.diff(reads.read_off).max()) > (64 if p_n < 0.1 else 140)
    sel = _pick(np.random.default_rng(3), g.tree.n_nodes, 300)
    ot = oracle.OracleTree(g.tree)
    D = am.oracle_distances(ot, reads)
    ot.close()
    mat = w.Mat(g.tree)
    got = mat.epp_assign(reads, GENOME, sel, want_bits=True)
    am.check_equal(got, am.assign_from_distances(lambda r: D[r, sel], 300, reads, GENOME), p_n)
    mat.close()


def _raw_call(mat, reads, genome, sel, cap, with_sel_buffer=True):
    """the C entry point itself (the binding calls again on WEPP_ELIMIT): (code, outputs)"""
    R, K = reads.n_reads, len(sel)
    sel = np.ascontiguousarray(sel, np.uint32)
    md = np.zeros(max(R, 1), np.int32); ne = np.zeros(max(R, 1), np.uint32)
    aoff = np.full(R + 1, 77, np.uint64); asel = np.zeros(max(cap, 1), np.uint32)
    sr = np.full(K, 9, np.uint32); sd = np.full(K, 9, np.int64); sc = np.full(K, 9, np.uint32)
    bits = np.full((K, (genome + 31) // 32), 9, np.uint32)
    rw = reads.read_word if reads.read_word.size else np.zeros(1, np.uint32)
    rd = _lib.EppReadsC(R, reads.read_off.ctypes.data, rw.ctypes.data, reads.start.ctypes.data, reads.end.ctypes.data,
                        reads.degree.ctypes.data)
    o = _lib.AssignOutC(md.ctypes.data, ne.ctypes.data, aoff.ctypes.data, asel.ctypes.data if with_sel_buffer else None, cap,
                        sr.ctypes.data, sd.ctypes.data, sc.ctypes.data, bits.ctypes.data)
    rc = _lib.lib.wepp_epp_assign(mat._h, ctypes.byref(rd), genome, K, sel.ctypes.data_as(ctypes.c_void_p), ctypes.byref(o))
    return rc, dict(min_dist=md[:R], n_epp=ne[:R], asg_off=aoff, asg_sel=asel[:int(aoff[R])] if rc == 0 else asel[:0],
                    sel_reads=sr, sel_degree=sd, sel_covered=sc, cover_bits=bits)


def test_capacity_protocol():
    rng = np.random.default_rng(4243)
    genome = 60
    tree, ref = ft.random_tree(rng, genome=genome, n_nodes=60)
    reads = epp_fuzz.random_epp_reads(rng, tree, ref, genome, n_reads=300)
    sel = _pick(rng, 60, 40)
    mat = w.Mat(tree)
    want = am.assign(tree, reads, genome, sel)
    need = int(want["asg_off"][-1])
    assert need > 300
    for cap in (0, 1, need - 1):
        rc, got = _raw_call(mat, reads, genome, sel, cap)
        assert rc == 4 and "call again" in _lib.lib.wepp_last_error().decode()
        for k in ("min_dist", "n_epp", "asg_off", "sel_reads", "sel_degree", "sel_covered", "cover_bits"):
            assert np.array_equal(got[k], want[k]), (cap, k)
    rc, got = _raw_call(mat, reads, genome, sel, 0, with_sel_buffer=False)      # the size query
    assert rc == 4 and int(got["asg_off"][-1]) == need
    rc, got = _raw_call(mat, reads, genome, sel, need)
    assert rc == 0
    am.check_equal(got, want, "exact capacity")
    am.check_equal(mat.epp_assign(reads, genome, sel, want_bits=True, asg_capacity=3), want, "binding retries")
    # no reads
    empty = w.EppReads.from_lists([], [], [])
    rc, got = _raw_call(mat, empty, genome, sel, 4)
    assert rc == 0 and got["asg_off"][0] == 0
    assert not got["sel_reads"].any() and not got["sel_degree"].any() and not got["sel_covered"].any() and not got["cover_bits"].any()
    # argument errors that need the handle
    with pytest.raises(w.WeppError) as ei:
        mat.epp_assign(reads, genome, [0, 60])
    assert ei.value.code == 1 and "not an arena index" in str(ei.value)
    with pytest.raises(w.WeppError) as ei:
        mat.epp_assign(reads, 0, [0])
    assert ei.value.code == 1 and "genome_size" in str(ei.value)
    bad = w.EppReads.from_lists([[(3, w.A, w.A)]], [1], [10])
    with pytest.raises(w.WeppError) as ei:
        mat.epp_assign(bad, genome, [0])
    assert "must differ from the reference base" in str(ei.value)
    assert mat.epp_assign(reads, 7, [0], want_lists=False)["sel_covered"][0] <= 7      # no 50-bin rule here
    mat.close()
    # a single-node tree
    tree = w.Tree.from_lists([-1], [[]])
    rd = w.EppReads.from_lists([[], [(7, w.A, w.N, 1)], [(9, w.C, w.T)], []], start=[1, 5, 9, 60], end=[60, 9, 9, 60], degree=[1, 2, 0, 5])
    mat = w.Mat(tree)
    got = mat.epp_assign(rd, 60, [0], want_bits=True)
    am.check_equal(got, am.assign(tree, rd, 60, [0]), "single node")
    assert got["min_dist"].tolist() == [0, 0, 1, 0] and got["sel_reads"][0] == 4 and got["sel_degree"][0] == 8
    assert got["sel_covered"][0] == 60      # the N at 7 of the second read lies under the first read
    mat.close()


def test_run_to_run_identical_and_the_map_in_between(oracle):
    g = w.generate_tree(9, 5000)
    reads = g.reads(10, 2000, windows=True, max_degree=3)
    sel = _pick(np.random.default_rng(1), 5000, 700)
    mat = w.Mat(g.tree)
    a = mat.epp_assign(reads, GENOME, sel, want_bits=True)
    m = mat.epp_map(reads, GENOME)                       # shares the handle's block cache
    b = mat.epp_assign(reads, GENOME, sel, want_bits=True)
    am.check_equal(a, b, "second call")
    want = oracle.OracleTree(g.tree).epp_map(reads, genome_size=GENOME)
    for k in ("max_parsimony", "multiplicity", "epp_off", "epp_nodes", "counts"):
        assert np.array_equal(m[k], want[k]), k
    mat.close()


def test_limits():
    """16-bit prefix counts and the 1 GiB table: a chain of five nodes with 14 000 mutations each under 5 000 leaves"""
    per = 14000
    parent = [-1, 0, 1, 2, 3] + [4] * 5000
    muts = [[(i * per + j + 1, w.A, w.A, w.C) for j in range(per)] for i in range(5)] + [[] for _ in range(5000)]
    tree = w.Tree.from_lists(parent, muts)
    mat = w.Mat(tree)
    order = mat.dfs_order()
    arena = {int(order[k]): k for k in range(5)}       # arena index of chain node i
    rd = w.EppReads.from_lists([[], [(3 * per + 1, w.A, w.C), (3 * per + 2, w.A, w.C)]], start=[1, 3 * per + 1], end=[5 * per, 3 * per + 2])
    got = mat.epp_assign(rd, 5 * per, [arena[3], arena[0]], want_lists=False)
    # an empty read over the whole genome is nearest to the haplotype with the fewest mutations (14 000 of them);
    # the second read repeats two mutations of chain node 3 (prefix counts beyond 42 000)
    assert got["min_dist"].tolist() == [per, 0] and got["n_epp"].tolist() == [1, 1]
    assert got["sel_reads"].tolist() == [1, 1] and got["sel_covered"].tolist() == [2, 5 * per]
    with pytest.raises(w.WeppError) as ei:
        mat.epp_assign(rd, 5 * per, [arena[4]])
    assert ei.value.code == 4 and "65535" in str(ei.value)
    with pytest.raises(w.WeppError) as ei:
        mat.epp_assign(rd, 5 * per, np.arange(4900, dtype=np.uint32))
    assert ei.value.code == 4 and "1 GiB" in str(ei.value)
    mat.close()
