"""wepp_epp_resolve on the GPU against the sequential model of arena::resolve_unaccounted_mutations
(tests/resolve_model.py), the oracle's haplotype::mutation_distance on the model's modified reads, and
wepp_epp_assign on those reads.  Everything is integer: bit-exact.

Layout units whose two sides are covered below: 64 columns per ballot of the best pass, 256 columns (a slab) per
pass of the tally, 1024 columns in k_assign's registers, RES_CHUNK = 256 relations per workgroup of the tally,
RES_MAX_CHUNK_WGS = 64 workgroups per mutation (longer lists: the workgroups stride over the chunks), 127 window
entries between two flushes of k_assign's byte counters."""
import ctypes

import numpy as np
import pytest

import assign_model as am
import epp_fuzz
import fuzz_trees as ft
import resolve_cases as rc
import resolve_model as rm
import wepp_amd as w
from wepp_amd import _lib

pytestmark = pytest.mark.gpu

GENOME = 29903
RES_CHUNK = 256
RES_MAX_CHUNK_WGS = 64


def _pick(rng, n, K):
    return rng.permutation(n)[:K].astype(np.uint32)


def _resolve(mat, reads, genome, sel, residual, **kw):
    return mat.epp_resolve(reads, genome, sel, residual, want_tallies=True, **kw)


def test_fuzz_small_trees():
    rng = np.random.default_rng(31337)
    total = dict.fromkeys(rm.BRANCHES, 0)
    for it in range(40):
        genome = 60
        tree, ref = ft.random_tree(rng, genome=genome)
        reads = epp_fuzz.random_epp_reads(rng, tree, ref, genome, n_reads=int(rng.integers(1, 601)))
        n = tree.n_nodes
        K = min(n, [1, 2, 3, 63, 64, 65, n][it % 7])
        sel = _pick(rng, n, K)
        residual = rc.draw_residual(rng, reads, ref, genome, int(rng.integers(1, 25)))
        want = rm.resolve(tree, reads, genome, sel, residual)
        for k, v in want["branches"].items():
            total[k] += v
        mat = w.Mat(tree)
        rm.check_equal(_resolve(mat, reads, genome, sel, residual), want, (it, K))
        mat.close()
    assert all(v > 0 for v in total.values()), total


HAND = rc.hand_cases()


def test_hand_cases():
    """two alleles at one position in both orders, insertions, window bounds, positions beyond the tree's last one, a
    mutation without reads, reads of degree 0 only, sums beyond 2^32, no touched read"""
    mats = {}
    for name, tree, reads, genome, sel, residual in HAND:
        mat = mats.setdefault(id(tree), w.Mat(tree))
        want = rm.resolve(tree, reads, genome, sel, residual)
        got = _resolve(mat, reads, genome, sel, residual)
        rm.check_equal(got, want, name)
        if name.startswith("int64") and len(sel) == 4:
            assert int(got["best_degree"][0]) == 3 * (2**31 - 1) and int(got["hap_degree"][1].max()) == 4 * (2**31 - 1)
        if name.startswith("degree 0") and len(sel) == 4:
            assert int(got["best_degree"][0]) == 0 and got["best"][0].tolist() == [1, 2]
        if name.startswith("untouched"):
            assert got["n_touched"] == 0 and not got["rel_off"].any() and not got["best_mask"].any()
            assert w.epp_resolve_last_timing()["assign_ms"] == 0.0          # no assignment was launched
    for mat in mats.values():
        mat.close()


@pytest.fixture(scope="module")
def layout_case(oracle):
    """per (tree size, residual list): the tree, the reads, the model's marking and the oracle's [reads, haplotypes]
    distances of the modified reads, computed once"""
    cache, mats = {}, {}

    def get(n_nodes, M):
        if (n_nodes, M) not in cache:
            g = w.generate_tree(11, n_nodes)
            reads = g.reads(12, 300, read_len=150, p_substitution=0.003, p_n=0.01, windows=True, max_degree=5)
            residual = rc.draw_residual(np.random.default_rng(M), reads, rc.reference_of(g, reads), GENOME, M)[:M]
            modified, covered, masked, _ = rm.mask_reads(reads, residual)
            ot = oracle.OracleTree(g.tree)
            D = am.oracle_distances(ot, modified)
            ot.close()
            if n_nodes not in mats:
                mats[n_nodes] = w.Mat(g.tree)
            cache[(n_nodes, M)] = (g, reads, residual, modified, covered, masked, D, mats[n_nodes])
        return cache[(n_nodes, M)]
    yield get
    for mat in mats.values():
        mat.close()


@pytest.mark.parametrize("n_nodes,K,M", [(600, k, 40) for k in (255, 256, 257)] + [(1100, k, 40) for k in (1023, 1025)] +
                         [(600, 257, m) for m in (1, 2, 300)])
def test_layout_edges(layout_case, n_nodes, K, M):
    g, reads, residual, modified, covered, masked, D, mat = layout_case(n_nodes, M)
    assert len(residual) == M
    sel = _pick(np.random.default_rng(K), n_nodes, K)
    want = rm.tally(modified, covered, masked, K, lambda r: D[r, sel])
    if M > 1:
        assert want["n_touched"] > 0
    rm.check_equal(_resolve(mat, reads, GENOME, sel, residual), want, (K, M))
    if want["n_touched"]:
        t = w.epp_resolve_last_timing()
        assert t["mark_ms"] > 0 and t["tables_ms"] > 0 and t["assign_ms"] > 0 and t["tally_ms"] > 0


@pytest.mark.parametrize("n_reads", [RES_CHUNK - 1, RES_CHUNK, RES_CHUNK + 1, RES_CHUNK * RES_MAX_CHUNK_WGS + 300])
def test_relation_list_around_a_chunk(n_reads):
    """one list of n_reads relations: one workgroup, two that meet in atomics, and more chunks than workgroups"""
    tree, reads, genome, sel, residual = rc.long_list_case(n_reads)
    want = rm.resolve(tree, reads, genome, sel, residual)
    assert int(want["n_covered"][1]) == n_reads
    mat = w.Mat(tree)
    rm.check_equal(_resolve(mat, reads, genome, sel, residual, rel_capacity=n_reads), want, n_reads)
    mat.close()


def _raw_call(mat, reads, genome, sel, res, cap, with_rel_buffer=True, tallies=True):
    """the C entry point itself (the binding calls again on WEPP_ELIMIT): (code, outputs)"""
    R, K, M = reads.n_reads, len(sel), len(res)
    sel = np.ascontiguousarray(sel, np.uint32)
    res = np.ascontiguousarray(res, np.uint32)
    roff = np.full(M + 1, 77, np.uint64); rrel = np.zeros(max(cap, 1), np.uint32)
    ncov = np.full(max(M, 1), 9, np.uint32); nmask = np.full(max(M, 1), 9, np.uint32); bdeg = np.full(max(M, 1), 9, np.int64)
    bmask = np.full((max(M, 1), (K + 31) // 32), 9, np.uint32)
    hr = np.full((max(M, 1), K), 9, np.uint32); hd = np.full((max(M, 1), K), 9, np.int64); nt = np.full(1, 9, np.uint32)
    rw = reads.read_word if reads.read_word.size else np.zeros(1, np.uint32)
    rd = _lib.EppReadsC(R, reads.read_off.ctypes.data, rw.ctypes.data, reads.start.ctypes.data, reads.end.ctypes.data,
                        reads.degree.ctypes.data)
    o = _lib.ResolveOutC(roff.ctypes.data, rrel.ctypes.data if with_rel_buffer else None, cap, ncov.ctypes.data, nmask.ctypes.data,
                         bdeg.ctypes.data, bmask.ctypes.data, hr.ctypes.data if tallies else None, hd.ctypes.data if tallies else None,
                         nt.ctypes.data)
    code = _lib.lib.wepp_epp_resolve(mat._h, ctypes.byref(rd), genome, K, sel.ctypes.data_as(ctypes.c_void_p), M,
                                     res.ctypes.data_as(ctypes.c_void_p) if M else None, ctypes.byref(o))
    bits = np.unpackbits(bmask[:M].view(np.uint8), axis=1, bitorder="little")[:, :K]
    return code, dict(rel_off=roff, rel_read=rrel[:int(roff[M])] if code == 0 else rrel[:0], n_covered=ncov[:M], n_masked=nmask[:M],
                      best_degree=bdeg[:M], best_mask=bmask[:M], best=[np.flatnonzero(b).astype(np.uint32) for b in bits],
                      hap_reads=hr[:M], hap_degree=hd[:M], n_touched=int(nt[0]))


def _words(residual):
    return np.array([int(w.pack_read_word(p, r, m)) for p, r, m in residual], np.uint32)


def test_capacity_protocol_and_empty_inputs():
    rng = np.random.default_rng(4244)
    genome = 60
    tree, ref = ft.random_tree(rng, genome=genome, n_nodes=60)
    reads = epp_fuzz.random_epp_reads(rng, tree, ref, genome, n_reads=300)
    sel = _pick(rng, 60, 40)
    residual = rc.draw_residual(rng, reads, ref, genome, 20)
    res = _words(residual)
    mat = w.Mat(tree)
    want = rm.resolve(tree, reads, genome, sel, residual)
    need = int(want["rel_off"][-1])
    assert need > 100
    others = [k for k in rm.KEYS if k != "rel_read"]
    for cap in (0, need - 1):
        code, got = _raw_call(mat, reads, genome, sel, res, cap)
        assert code == 4 and "call again" in _lib.lib.wepp_last_error().decode()
        for k in others:
            assert np.array_equal(got[k], want[k]), (cap, k)
        assert got["n_touched"] == want["n_touched"]
    code, got = _raw_call(mat, reads, genome, sel, res, 0, with_rel_buffer=False)       # the size query
    assert code == 4 and int(got["rel_off"][-1]) == need
    code, got = _raw_call(mat, reads, genome, sel, res, need)
    assert code == 0
    rm.check_equal(got, want, "exact capacity")
    code, got = _raw_call(mat, reads, genome, sel, res, need, tallies=False)            # hap_reads / hap_degree may be NULL
    assert code == 0 and np.array_equal(got["best_mask"], want["best_mask"]) and (got["hap_reads"] == 9).all()
    rm.check_equal(_resolve(mat, reads, genome, sel, residual, rel_capacity=3), want, "binding retries")
    lists_only = mat.epp_resolve(reads, genome, sel, res)                               # packed words, no tallies
    assert np.array_equal(lists_only["rel_read"], want["rel_read"]) and "hap_reads" not in lists_only
    # n_res == 0, no reads
    code, got = _raw_call(mat, reads, genome, sel, res[:0], 4)
    assert code == 0 and got["rel_off"].tolist() == [0] and got["n_touched"] == 0
    empty = w.EppReads.from_lists([], [], [])
    code, got = _raw_call(mat, empty, genome, sel, res, 4)
    assert code == 0 and not got["rel_off"].any() and got["n_touched"] == 0
    for k in ("n_covered", "n_masked", "best_degree", "best_mask", "hap_reads", "hap_degree"):
        assert not got[k].any(), k
    assert w.epp_resolve_last_timing() == dict(mark_ms=0.0, tables_ms=0.0, assign_ms=0.0, tally_ms=0.0)
    mat.close()


def test_argument_errors():
    tree, ref = rc.hand_tree()
    reads = w.EppReads.from_lists([[(5, w.A, w.C)], []], [1, 10], [30, 40])
    mat = w.Mat(tree)
    for residual, what in (([(0, w.A, w.C)], "outside 1 .. genome_size"), ([(61, w.A, w.C)], "outside 1 .. genome_size"),
                           ([(5, w.A, 0)], "mut_nuc"), ([(5, w.A, 15)], "mut_nuc"), ([(5, w.A | w.C, w.C)], "one-hot"),
                           ([(5, 0, w.C)], "one-hot"), ([(5, w.A, w.C), (7, w.A, w.N)], "residual mutation 1")):
        with pytest.raises(w.WeppError) as ei:
            mat.epp_resolve(reads, 60, [0, 1], residual)
        assert ei.value.code == 1 and what in str(ei.value), residual
    # the checks of wepp_epp_assign, same codes and messages
    with pytest.raises(w.WeppError) as ei:
        mat.epp_resolve(reads, 60, [0, 4], [(5, w.A, w.C)])
    assert ei.value.code == 1 and "not an arena index" in str(ei.value)
    with pytest.raises(w.WeppError) as ei:
        mat.epp_resolve(reads, 0, [0], [(5, w.A, w.C)])
    assert ei.value.code == 1 and "genome_size" in str(ei.value)
    bad = w.EppReads.from_lists([[(3, w.A, w.A)]], [1], [10])
    with pytest.raises(w.WeppError) as ei:
        mat.epp_resolve(bad, 60, [0], [(5, w.A, w.C)])
    assert "must differ from the reference base" in str(ei.value)
    mat.close()


def test_run_to_run_identical_with_assign_and_map_in_between():
    g = w.generate_tree(9, 5000)
    reads = g.reads(10, 2000, windows=True, max_degree=3)
    sel = _pick(np.random.default_rng(1), 5000, 700)
    residual = rc.draw_residual(np.random.default_rng(2), reads, rc.reference_of(g, reads), GENOME, 200)
    mat = w.Mat(g.tree)
    a = _resolve(mat, reads, GENOME, sel, residual)
    asg = mat.epp_assign(reads, GENOME, sel)            # both share the handle's block cache
    mat.epp_map(reads, GENOME)
    b = _resolve(mat, reads, GENOME, sel, residual)
    rm.check_equal(a, b, "second call")
    assert a["n_touched"] > 100
    assert np.array_equal(mat.epp_assign(reads, GENOME, sel)["asg_sel"], asg["asg_sel"])
    mat.close()


def test_against_epp_assign_on_the_modified_reads():
    """a cross-check without the model's distances: the device's own assignment of the model's modified reads, tallied
    in NumPy"""
    g = w.generate_tree(7, 3000)
    reads = g.reads(8, 1500, windows=True, max_degree=4, p_n=0.02)
    K = 500
    sel = _pick(np.random.default_rng(5), 3000, K)
    residual = rc.draw_residual(np.random.default_rng(6), reads, rc.reference_of(g, reads), GENOME, 150)
    M = len(residual)
    modified, covered, masked, count = rm.mask_reads(reads, residual)
    assert all(count[k] > 0 for k in ("entry_match", "entry_n", "absent_ref"))
    mat = w.Mat(g.tree)
    asg = mat.epp_assign(modified, GENOME, sel)
    tie = np.zeros((reads.n_reads, K), bool)
    rows = np.repeat(np.arange(reads.n_reads), np.diff(asg["asg_off"]).astype(np.int64))
    tie[rows, asg["asg_sel"]] = True
    hr = np.zeros((M, K), np.uint32); hd = np.zeros((M, K), np.int64)
    for m in range(M):
        rs = np.array(sorted(covered[m] + masked[m]), np.int64)
        if rs.size:
            hr[m] = tie[rs].sum(axis=0)
            hd[m] = (tie[rs] * modified.degree[rs].astype(np.int64)[:, None]).sum(axis=0)
    got = _resolve(mat, reads, GENOME, sel, residual)
    assert np.array_equal(got["hap_reads"], hr) and np.array_equal(got["hap_degree"], hd)
    assert np.array_equal(got["n_covered"], [len(c) for c in covered]) and np.array_equal(got["n_masked"], [len(c) for c in masked])
    mat.close()


def test_long_reads():
    """1 200 bp at 20 % N: more than 127 entries inside the window of a modified read"""
    g = w.generate_tree(5, 8000)
    reads = g.reads(21, 30, read_len=1200, amplicon_len=1200, amplicon_step=1000, p_substitution=0.003, p_n=0.2,
                    windows=True, max_degree=3)
    sel = _pick(np.random.default_rng(3), g.tree.n_nodes, 300)
    residual = rc.draw_residual(np.random.default_rng(4), reads, rc.reference_of(g, reads), GENOME, 120)
    want = rm.resolve(g.tree, reads, GENOME, sel, residual)
    assert want["branches"]["absent_ref"] > 0 and want["n_touched"] > 10
    mod = want["modified"]
    grown = np.diff(mod.read_off).astype(np.int64) - np.diff(reads.read_off).astype(np.int64)
    assert grown.max() > 0 and int(np.diff(mod.read_off)[grown > 0].max()) > 140
    mat = w.Mat(g.tree)
    rm.check_equal(_resolve(mat, reads, GENOME, sel, residual), want, "long")
    mat.close()
