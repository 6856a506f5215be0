"""wepp_mat_set_clades / wepp_clade_assign on the GPU against tests/clades_model.py fed with the ORACLE's optimal
nodes: wepp_place_batch, then wepp_best_nodes, then wepp_clade_assign; best_clade, hist_off, hist_clade and hist_count
bit for bit.

Paths of a segment (the pairs of one read in one column, clades.hpp): 1 key (no sort), 2 .. 64 (a wave), 65 .. 1024
(a workgroup), more (the device radix sort): 1, 2, 63, 64, 65, 1023, 1024, 1025 and 4100 keys below."""
import ctypes

import numpy as np
import pytest

import clades_cases as cc
import fuzz_trees as ft
import wepp_amd as w
from wepp_amd import _lib
from wepp_amd.api import _ptr

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4100]


def _run(mat, reads):
    res = mat.place_batch(reads)
    off, nodes = mat.best_nodes_csr(reads, res)
    return res, off, nodes, mat.clade_assign(reads, res, off, nodes)


def _check(got, want, tag):
    bc, hoff, hc, hn = got
    assert np.array_equal(bc, want[0]), tag
    assert np.array_equal(hoff, want[1]), tag
    assert np.array_equal(hc, want[2]), tag
    assert np.array_equal(hn, want[3]), tag


@pytest.fixture(scope="module")
def hub(oracle):
    """The hub tree, a batch that mixes every segment size with reads without entries, and the oracle's optimal nodes"""
    tree, info = cc.hub_tree(SIZES)
    rng = np.random.default_rng(4242)
    samples = []
    for g in info["groups"]:
        samples += [g["sample"], []]
    samples += [info["probe_shared"], info["probe_unique"], [], [(5, cc.A, cc.C, 0), (10, cc.A, cc.C, 0)], [(11, cc.A, cc.G, 0)]]
    order = rng.permutation(len(samples))
    samples = [samples[int(i)] for i in order]
    ot = oracle.OracleTree(tree)
    best = cc.oracle_best(ot, samples)
    ot.close()
    # a hub of H leaves that all carry the sample's mutation: H optimal nodes, by the oracle
    by_sample = {tuple(s): b for s, b in zip(samples, best)}
    for g in info["groups"]:
        assert by_sample[tuple(g["sample"])][1] == g["size"]
    mat = w.Mat(tree)
    yield dict(tree=tree, info=info, samples=samples, best=best, reads=cc.reads_of(samples), mat=mat)
    mat.close()


@pytest.mark.parametrize("pattern", ["none", "root", "all", "mixed"])
@pytest.mark.parametrize("n_columns", [1, 2, 8])
def test_hub_segments(hub, n_columns, pattern):
    tree, info = hub["tree"], hub["info"]
    parent = [int(p) for p in tree.parent]
    columns = cc.annotate(info["kind"], parent, n_columns, pattern, np.random.default_rng(n_columns))
    want = cc.expected(tree, columns, hub["samples"], hub["best"])
    per_sample, pairs = want[4], want[5]
    # the inputs hold what this test is about (asserted on the model and the oracle, not on the code under test)
    seg = set(len(p) for p in pairs)
    assert set(SIZES) <= seg
    assert any(len(s) == 0 for s in hub["samples"])
    if pattern == "none":
        assert all(b == "UNDEFINED" and set(names) == {"UNDEFINED"} for out in per_sample for (b, names) in out)
    if pattern == "mixed":
        assert any(info["kind"][n] == "leaf" and columns[0][n] != "" and not inc for pr in pairs for (n, inc, _u) in pr)
        probe = [(inc, u) for pr in pairs for (n, inc, u) in pr if n == info["probe"]]
        assert (True, False) in probe and (False, True) in probe
        shared = per_sample[hub["samples"].index(info["probe_shared"])][0]
        unique = per_sample[hub["samples"].index(info["probe_unique"])][0]
        assert shared[0] == "PROBE" and unique[0] != "PROBE"
        assert any(len(cc.cm.run_lengths(names)) > 2 for out in per_sample for (_b, names) in out)
    mat = hub["mat"]
    cid, und, _names = w.number_clade_names(columns)
    mat.set_clades(cid, und)
    res, off, nodes, got = _run(mat, hub["reads"])
    assert [int(x) for x in res.best_bfs_j] == [b[0] for b in hub["best"]]
    assert [int(x) for x in nodes] == [j for b in hub["best"] for j in b[2]]
    _check(got, want, (n_columns, pattern))
    hoff, R = got[1].astype(np.int64), hub["reads"].n_reads
    for s in range(n_columns * R):                     # the counts of a segment sum to num_best
        assert int(got[3][hoff[s]:hoff[s + 1]].sum()) == hub["best"][s % R][1]
    t = w.clade_last_timing()
    assert t["pairs_ms"] > 0


def test_fuzz_trees(oracle):
    rng = np.random.default_rng(777)
    kinds = dict(leaf_annotated=0, internal_incl=0, internal_excl=0, undefined=0, multi_run=0, both=0)
    for it in range(36):
        tree, ref = ft.random_tree(rng, n_nodes=int(rng.integers(1, 300)), genome=40, max_muts=2)
        parent, _muts = cc.cm.tree_lists(tree)
        _bfs, kids = cc.cm.bfs_order(parent)
        n = tree.n_nodes
        n_columns = [1, 2, 8][it % 3]
        pattern = ["none", "root", "all", "random"][(it // 3) % 4]
        if pattern == "random":
            columns = [[cc.POOL[int(rng.integers(0, len(cc.POOL)))] if rng.random() < 0.4 else "" for _ in range(n)]
                       for _ in range(n_columns)]
        else:
            columns = cc.annotate(["root" if p < 0 else "node" for p in parent], parent, n_columns, pattern, rng)
        samples = [ft.random_sample(rng, ref, genome=40, max_k=4) for _ in range(40)]
        ot = oracle.OracleTree(tree)
        best = cc.oracle_best(ot, samples)
        ot.close()
        want = cc.expected(tree, columns, samples, best)
        seen_hu = {}
        for out, pr in zip(want[4], want[5]):
            for (node, inc, u) in pr:
                if not kids[node] and columns[0][node] != "":
                    kinds["leaf_annotated"] += 1
                if kids[node] and columns[0][node] != "":
                    kinds["internal_incl" if inc else "internal_excl"] += 1
                    seen_hu.setdefault(node, set()).add(u)
            kinds["undefined"] += sum(1 for (b, _n) in out if b == "UNDEFINED")
            kinds["multi_run"] += sum(1 for (_b, names) in out if len(set(names)) > 1)
        kinds["both"] += sum(1 for v in seen_hu.values() if len(v) == 2)
        mat = w.Mat(tree)
        cid, und, _names = w.number_clade_names(columns)
        mat.set_clades(cid, und)
        res, off, nodes, got = _run(mat, cc.reads_of(samples))
        assert [int(x) for x in res.best_bfs_j] == [b[0] for b in best]
        assert [int(x) for x in nodes] == [j for b in best for j in b[2]]
        _check(got, want, (it, n_columns, pattern))
        # the histograms are optional: best_clade alone
        only = mat.clade_assign(cc.reads_of(samples), res, off, nodes, want_hist=False)
        assert np.array_equal(only[0], want[0])
        mat.close()
    assert all(v > 0 for v in kinds.values()), kinds


def _raw(mat, reads, res, off, nodes, C, capacity, best_bfs_j=None):
    n = reads.n_reads
    bc = np.full((C, n), 0xFFFFFFFF, np.uint32)
    hoff = np.zeros(C * n + 1, np.uint64)
    hc = np.zeros(max(capacity, 1), np.uint32); hn = np.zeros(max(capacity, 1), np.uint32)
    bj = np.ascontiguousarray(res.best_bfs_j if best_bfs_j is None else best_bfs_j, np.uint32)
    rc = _lib.lib.wepp_clade_assign(mat._h, _ptr(reads.read_off), _ptr(reads.read_word), n, _ptr(bj), _ptr(off), _ptr(nodes),
                                    _ptr(bc), _ptr(hoff), _ptr(hc), _ptr(hn), capacity)
    return rc, bc, hoff, hc, hn


def test_errors(hub):
    tree, info = hub["tree"], hub["info"]
    parent = [int(p) for p in tree.parent]
    reads = hub["reads"]
    fresh = w.Mat(tree)
    res = fresh.place_batch(reads)
    off, nodes = fresh.best_nodes_csr(reads, res)
    # no clades set
    rc, *_ = _raw(fresh, reads, res, off, nodes, 1, 0)
    assert rc == 1 and b"no clades set" in _lib.lib.wepp_last_error()
    # 9 columns
    cols9 = cc.annotate(info["kind"], parent, 9, "root", np.random.default_rng(0))
    cid, und, _ = w.number_clade_names(cols9)
    with pytest.raises(w.WeppError) as e:
        fresh.set_clades(cid, und)
    assert e.value.code == 4
    rc, *_ = _raw(fresh, reads, res, off, nodes, 1, 0)
    assert rc == 1                                     # (the refused call set nothing)
    # capacity one too small: the sizes and best_clade are delivered
    columns = cc.annotate(info["kind"], parent, 2, "mixed", np.random.default_rng(2))
    want = cc.expected(tree, columns, hub["samples"], hub["best"])
    cid, und, _ = w.number_clade_names(columns)
    fresh.set_clades(cid, und)
    need = int(want[1][-1])
    rc, bc, hoff, _hc, _hn = _raw(fresh, reads, res, off, nodes, 2, need - 1)
    assert rc == 4
    assert int(hoff[-1]) == need and np.array_equal(hoff, want[1])
    assert np.array_equal(bc, want[0])
    rc, bc, hoff, hc, hn = _raw(fresh, reads, res, off, nodes, 2, need)
    assert rc == 0
    _check((bc, hoff, hc[:need], hn[:need]), want, "exact capacity")
    # a best_bfs_j that is not among the read's nodes
    r = next(i for i, b in enumerate(hub["best"]) if b[1] == 2)
    wrong = res.best_bfs_j.copy()
    wrong[r] = next(j for j in range(tree.n_nodes) if j not in hub["best"][r][2])
    rc, *_ = _raw(fresh, reads, res, off, nodes, 2, need, best_bfs_j=wrong)
    assert rc == 1 and b"not among" in _lib.lib.wepp_last_error()
    # a best_nodes entry that is no BFS index
    bad = nodes.copy()
    bad[len(bad) // 2] = tree.n_nodes
    rc, *_ = _raw(fresh, reads, res, off, bad, 2, need)
    assert rc == 1 and b"not a BFS index" in _lib.lib.wepp_last_error()
    # zero columns clears the tables
    fresh.set_clades(np.zeros((0, tree.n_nodes), np.uint32), np.zeros(0, np.uint32))
    rc, *_ = _raw(fresh, reads, res, off, nodes, 2, need)
    assert rc == 1
    fresh.close()
