"""wepp_epp_neighbors / wepp_epp_distances on the GPU against the literal model of arena::closest_neighbors and
arena::highest_scoring_neighbors (tests/neighbors_model.py: list merges, BFS, climb + DFS).  Everything is integer:
bit-exact, lists, distances, tops and region sizes.

Layout units whose two sides are covered below (neighbors.hpp): 4 pivot columns per lane, 256 per wave and row load,
256 rows per block of the column scans, the row N that takes the deltas of subtrees ending with the tree, several
passes over the pivots."""
import ctypes

import numpy as np
import pytest

import neighbors_model as nm
import wepp_amd as w
from wepp_amd import _lib

pytestmark = pytest.mark.gpu

TO, FROM = nm.TO, nm.FROM


def _sub(want, K):
    """the first K pivots of a model result"""
    n = int(want["nbr_off"][K])
    return dict(nbr_off=want["nbr_off"][:K + 1], nbr_node=want["nbr_node"][:n], nbr_dist=want["nbr_dist"][:n],
                top=want["top"][:K], n_region=want["n_region"][:K])


def test_fuzz_small_trees():
    total = partial = 0
    for it, (tree, ar, piv) in enumerate(nm.fuzz_cases()):
        mat = w.Mat(tree)
        for form in (TO, FROM):
            want_d = np.array([ar.field(int(p), form) for p in piv], np.int32)
            assert np.array_equal(mat.epp_distances(piv, form), want_d), (it, form)
            for radius in nm.FUZZ_RADII:
                want = ar.neighbors(piv, radius, form)
                nm.check_equal(mat.epp_neighbors(piv, radius, form), want, (it, form, radius))
                total += len(piv)
                partial += int(((want["n_region"] > 1) & (want["n_region"] < ar.n)).sum())
        skip = (np.arange(ar.n) % 3 == 1).astype(np.uint8)
        nm.check_equal(mat.epp_neighbors(piv, 2, FROM, skip=skip), ar.neighbors(piv, 2, FROM, skip), (it, "skip"))
        mat.close()
    # not vacuous: regions that are neither the pivot alone nor the whole tree (tests/test_neighbors_model.py shows
    # the same on the model alone)
    assert 3 * partial >= total, (partial, total)


@pytest.mark.parametrize("name", sorted(nm.hand_cases()))
def test_hand_cases(name):
    tree, piv, radius, skip, lists = nm.hand_cases()[name]
    ar = nm.Arena(tree)
    mat = w.Mat(tree)
    for form in (TO, FROM):
        got = mat.epp_neighbors(piv, radius, form, skip=skip)
        nm.check_equal(got, ar.neighbors(piv, radius, form, skip), (name, form))
        assert [got["nbr_node"][int(got["nbr_off"][i]):int(got["nbr_off"][i + 1])].tolist() for i in range(len(piv))] == lists[form]
    mat.close()


LAYOUT_RADIUS = 2


@pytest.fixture(scope="module")
def tree600():
    """a 600-node generated tree, 257 pivots and the model's regions of them, computed once"""
    g = w.generate_tree(11, 600)
    ar = nm.Arena(g.tree)
    piv = np.random.default_rng(257).permutation(600)[:257].astype(np.uint32)
    want = {form: ar.neighbors(piv, LAYOUT_RADIUS, form) for form in (TO, FROM)}
    return g.tree, ar, piv, want


@pytest.mark.parametrize("K", [1, 255, 256, 257])
def test_pivot_column_edges(tree600, K):
    tree, ar, piv, want = tree600
    mat = w.Mat(tree)
    for form in (TO, FROM):
        nm.check_equal(mat.epp_neighbors(piv[:K], LAYOUT_RADIUS, form), _sub(want[form], K), (K, form))
    # the field of the pivots next to the slab edge
    some = piv[max(0, K - 3):K]
    assert np.array_equal(mat.epp_distances(some, FROM), np.array([ar.field(int(p), FROM) for p in some], np.int32))
    t = w.epp_neighbors_last_timing()
    assert t["tables_ms"] > 0 and t["field_ms"] > 0
    sizes = want[TO]["n_region"][:K]
    assert sizes.max() > 1
    mat.close()


@pytest.mark.parametrize("pass_cols", [1, 256])
def test_several_passes_equal_one(tree600, monkeypatch, pass_cols):
    tree, ar, piv, want = tree600
    monkeypatch.setenv("WEPP_NBR_PASS_COLS", str(pass_cols))       # (read by the handle's first call)
    mat = w.Mat(tree)
    for form in (TO, FROM):
        nm.check_equal(mat.epp_neighbors(piv, LAYOUT_RADIUS, form), want[form], (pass_cols, form))
    some = piv[254:257]
    assert np.array_equal(mat.epp_distances(some, TO), np.array([ar.field(int(p), TO) for p in some], np.int32))
    mat.close()


@pytest.mark.parametrize("n_nodes", [255, 256, 257, 513])
def test_scan_block_edges(n_nodes):
    g = w.generate_tree(11, n_nodes)
    ar = nm.Arena(g.tree)
    hub = nm.hub_leaf(ar)
    piv = np.unique(np.array([0, n_nodes - 1, n_nodes // 2, min(n_nodes - 1, 255), 254, 1, hub], np.uint32))
    mat = w.Mat(g.tree)
    for form in (TO, FROM):
        for radius in (1, 3):
            nm.check_equal(mat.epp_neighbors(piv, radius, form), ar.neighbors(piv, radius, form), (n_nodes, form, radius))
        assert np.array_equal(mat.epp_distances(piv, form), np.array([ar.field(int(p), form) for p in piv], np.int32))
    mat.close()


def _chain(n):
    """every node is an ancestor of the next; position 1 + i % 7 flips between reference and C every 7 nodes"""
    A, C = w.A, w.C
    fwd = lambda i: (i // 7) % 2 == 0
    return w.Tree.from_lists([-1] + list(range(n - 1)), [[(1 + i % 7, A, A if fwd(i) else C, C if fwd(i) else A)] for i in range(n)])


def _star(n):
    A, C, N = w.A, w.C, w.N
    return w.Tree.from_lists([-1] + [0] * (n - 1), [[]] + [[(1 + i % 5, A, A, N if i % 11 == 0 else C)] for i in range(n - 1)])


@pytest.mark.parametrize("shape", ["chain", "star"])
def test_chain_and_star(shape):
    n = 300
    tree = _chain(n) if shape == "chain" else _star(n)
    ar = nm.Arena(tree)
    piv = np.array([0, n - 1, 150, 1, 256, 255], np.uint32)
    mat = w.Mat(tree)
    sizes = []
    for form in (TO, FROM):
        for radius in (0, 1, 3):
            want = ar.neighbors(piv, radius, form)
            nm.check_equal(mat.epp_neighbors(piv, radius, form), want, (shape, form, radius))
            sizes += want["n_region"].tolist()
    assert any(1 < s < n for s in sizes)
    mat.close()


def _raw_call(mat, piv, radius, form, cap, skip=None, with_buffers=True, want_extra=True):
    """the C entry point itself (the binding calls again on WEPP_ELIMIT): (code, outputs)"""
    piv = np.ascontiguousarray(piv, np.uint32)
    K = piv.size
    off = np.full(K + 1, 77, np.uint64); node = np.full(max(cap, 1), 9, np.uint32); dist = np.full(max(cap, 1), 9, np.int32)
    top = np.full(max(K, 1), 9, np.uint32); nreg = np.full(max(K, 1), 9, np.uint32)
    o = _lib.NeighborsOutC(off.ctypes.data, node.ctypes.data if with_buffers else None, dist.ctypes.data if with_buffers else None,
                           cap, top.ctypes.data if want_extra else None, nreg.ctypes.data if want_extra else None)
    rc = _lib.lib.wepp_epp_neighbors(mat._h, K, piv.ctypes.data_as(ctypes.c_void_p) if K else None, radius, form,
                                     skip.ctypes.data_as(ctypes.c_void_p) if skip is not None else None, ctypes.byref(o))
    n = int(off[K]) if rc == 0 else 0
    return rc, dict(nbr_off=off, nbr_node=node[:n], nbr_dist=dist[:n], top=top[:K], n_region=nreg[:K]), (node, dist)


def test_capacity_protocol_and_arguments():
    tree, ar, piv = next(nm.fuzz_cases(1, seed=99))
    mat = w.Mat(tree)
    want = ar.neighbors(piv, 3, TO)
    need = int(want["nbr_off"][-1])
    assert need > len(piv)
    # the sizes only; a buffer one short: WEPP_ELIMIT, every other output intact
    for cap, buffers in ((0, False), (0, True), (need - 1, True)):
        rc, got, _ = _raw_call(mat, piv, 3, TO, cap, with_buffers=buffers)
        assert rc == 4 and "call again" in _lib.lib.wepp_last_error().decode()
        for k in ("nbr_off", "top", "n_region"):
            assert np.array_equal(got[k], want[k]), (cap, k)
    rc, got, _ = _raw_call(mat, piv, 3, TO, need)
    assert rc == 0
    nm.check_equal(got, want, "exact capacity")
    rc, got, _ = _raw_call(mat, piv, 3, TO, need + 5, want_extra=False)        # top / n_region may be NULL
    assert rc == 0 and np.array_equal(got["nbr_node"], want["nbr_node"]) and np.array_equal(got["nbr_dist"], want["nbr_dist"])
    nm.check_equal(mat.epp_neighbors(piv, 3, TO, nbr_capacity=1), want, "binding retries")
    # two identical calls: identical bytes, buffers beyond the lists untouched
    a = _raw_call(mat, piv, 2, FROM, need + 7)
    b = _raw_call(mat, piv, 2, FROM, need + 7)
    assert a[0] == 0 and b[0] == 0
    assert a[2][0].tobytes() == b[2][0].tobytes() and a[2][1].tobytes() == b[2][1].tobytes()
    for k in ("nbr_off", "top", "n_region"):
        assert a[1][k].tobytes() == b[1][k].tobytes()
    # every skipped pivot: nothing listed, WEPP_OK with no buffers at all
    skip = np.ones(ar.n, np.uint8)
    rc, got, _ = _raw_call(mat, piv[:1], 0, TO, 0, skip=skip, with_buffers=False)
    assert rc == 0 and got["nbr_off"].tolist() == [0, 0] and got["n_region"][0] >= 1
    # argument errors
    bad = [dict(piv=np.zeros(0, np.uint32)), dict(piv=[0, ar.n]), dict(piv=[1, 0, 1]), dict(piv=[0], form=2), dict(piv=[0], form=-1)]
    for kw in bad:
        with pytest.raises(w.WeppError) as ei:
            mat.epp_neighbors(kw["piv"], 1, kw.get("form", TO))
        assert ei.value.code == 1, kw
        if len(kw["piv"]):
            with pytest.raises(w.WeppError) as ei:
                mat.epp_distances(kw["piv"], kw.get("form", TO))
            assert ei.value.code == 1, kw
    assert _lib.lib.wepp_epp_neighbors(mat._h, 1, np.zeros(1, np.uint32).ctypes.data_as(ctypes.c_void_p), 1, TO, None, None) == 1
    assert _lib.lib.wepp_epp_neighbors(mat._h, 1, None, 1, TO, None, ctypes.byref(_lib.NeighborsOutC())) == 1
    assert _lib.lib.wepp_epp_neighbors(None, 1, np.zeros(1, np.uint32).ctypes.data_as(ctypes.c_void_p), 1, TO, None,
                                       ctypes.byref(_lib.NeighborsOutC(np.zeros(2, np.uint64).ctypes.data))) == 1
    assert _lib.lib.wepp_epp_distances(mat._h, 1, np.zeros(1, np.uint32).ctypes.data_as(ctypes.c_void_p), TO, None) == 1
    o = _lib.NeighborsOutC(np.zeros(2, np.uint64).ctypes.data, None, None, 4, None, None)     # a capacity without buffers
    assert _lib.lib.wepp_epp_neighbors(mat._h, 1, np.zeros(1, np.uint32).ctypes.data_as(ctypes.c_void_p), 1, TO, None, ctypes.byref(o)) == 1
    mat.close()
    # a single-node tree
    tree = w.Tree.from_lists([-1], [[(3, w.A, w.A, w.C)]])
    mat = w.Mat(tree)
    for form in (TO, FROM):
        got = mat.epp_neighbors([0], 0, form)
        assert got["nbr_node"].tolist() == [0] and got["nbr_dist"].tolist() == [0] and got["top"].tolist() == [0]
        assert mat.epp_distances([0], form).tolist() == [[0]]
    mat.close()


def test_field_cell_limit():
    g = w.generate_tree(3, 70000)
    mat = w.Mat(g.tree)
    with pytest.raises(w.WeppError) as ei:
        mat_piv = np.arange(3835, dtype=np.uint32)        # 3835 * 70000 > 2^28
        _lib.check(_lib.lib.wepp_epp_distances(mat._h, mat_piv.size, mat_piv.ctypes.data_as(ctypes.c_void_p), TO,
                                               np.zeros(1, np.int32).ctypes.data_as(ctypes.c_void_p)))
    assert ei.value.code == 4 and "2^28" in str(ei.value)
    # the whole tree within reach of a far radius: one pivot, every node
    got = mat.epp_neighbors([g.tree.n_nodes - 1], 10**6, FROM)
    assert got["n_region"].tolist() == [70000] and np.array_equal(got["nbr_node"], np.arange(70000, dtype=np.uint32))
    assert got["nbr_dist"][-1] == 0 and got["top"].tolist() == [0]
    mat.close()
