"""wepp_epp_neighbors / wepp_epp_distances without a GPU: the entry points' own host code (neighbors_capi.cpp,
epp_host.cpp: the pass loop, the handle's dfs_end) on neighbors_kernels.hip compiled as plain C++ and an emulated HIP
runtime (tests/epp_emu.py, tests/cxx/hip_emu: one host thread per lane), against the literal model
(tests/neighbors_model.py).  Checks the host side's and the kernels' logic, sizes and indexing; the device is the
business of tests/test_epp_neighbors_gpu.py."""
import numpy as np
import pytest

import epp_emu
import neighbors_model as nm
import wepp_amd as w

emu = epp_emu.neighbors


def test_fuzz_trees(monkeypatch):
    for it, (tree, ar, piv) in enumerate(nm.fuzz_cases(10)):
        for form in (nm.TO, nm.FROM):
            for radius in (0, 2):
                nm.check_equal(emu(tree, piv, radius, form), ar.neighbors(piv, radius, form), (it, form, radius))
            dist = epp_emu.distances(tree, piv, form)
            for i, p in enumerate(piv):
                assert np.array_equal(dist[i], ar.field(int(p), form)), (it, form, p)
        skip = (np.arange(ar.n) % 3 == 1).astype(np.uint8)
        nm.check_equal(emu(tree, piv, 2, nm.FROM, skip=skip), ar.neighbors(piv, 2, nm.FROM, skip), (it, "skip"))
        with monkeypatch.context() as mp:
            mp.setenv("WEPP_NBR_PASS_COLS", str(1 + it % 3))        # (read by the handle's first call: every call has its own)
            nm.check_equal(emu(tree, piv, 1, nm.TO), ar.neighbors(piv, 1, nm.TO), (it, "passes"))
            assert np.array_equal(epp_emu.distances(tree, piv, nm.TO), np.array([ar.field(int(p), nm.TO) for p in piv], np.int32))


@pytest.mark.parametrize("name", sorted(nm.hand_cases()))
def test_hand_cases(name):
    tree, piv, radius, skip, _ = nm.hand_cases()[name]
    ar = nm.Arena(tree)
    for form in (nm.TO, nm.FROM):
        nm.check_equal(emu(tree, piv, radius, form, skip=skip), ar.neighbors(piv, radius, form, skip), (name, form))


# both sides of the 256-row scan block, and more than 4 pivot columns in a pass; the 256-column slab is left to the GPU
@pytest.mark.parametrize("n_nodes", [255, 256, 257, 513])
def test_scan_block_edges(n_nodes):
    g = w.generate_tree(11, n_nodes, genome_len=3000)
    ar = nm.Arena(g.tree)
    # (np.unique, as in the GPU test: the entry point's own check refuses a pivot listed twice -- 254 of 255, 255 of 256)
    piv = np.unique(np.array([0, n_nodes - 1, n_nodes // 2, 255 if n_nodes > 255 else 7, 254, 1], np.uint32))
    for form in (nm.TO, nm.FROM):
        nm.check_equal(emu(g.tree, piv, 2, form), ar.neighbors(piv, 2, form), (n_nodes, form))
        assert np.array_equal(epp_emu.distances(g.tree, [n_nodes - 1], form)[0], ar.field(n_nodes - 1, form))


def test_chain_and_star():
    A, C = w.A, w.C
    chain = w.Tree.from_lists([-1] + list(range(39)), [[(1 + i % 7, A, A if (i // 7) % 2 == 0 else C, C if (i // 7) % 2 == 0 else A)] for i in range(40)])
    star = w.Tree.from_lists([-1] + [0] * 39, [[]] + [[(1 + i % 5, A, A, C)] for i in range(39)])
    for tree in (chain, star):
        ar = nm.Arena(tree)
        piv = np.array([0, 39, 20], np.uint32)
        for form in (nm.TO, nm.FROM):
            for radius in (0, 1, 3):
                nm.check_equal(emu(tree, piv, radius, form), ar.neighbors(piv, radius, form), (form, radius))


def test_capacity_protocol_and_arguments():
    tree, ar, piv = next(nm.fuzz_cases(1, seed=99))
    want = ar.neighbors(piv, 3, nm.TO)
    need = int(want["nbr_off"][-1])
    assert need > len(piv)
    for cap in (0, need - 1):
        with pytest.raises(w.WeppError) as ei:
            emu(tree, piv, 3, nm.TO, capacity=cap)
        assert ei.value.code == 4 and "hold %d entries, %d needed" % (cap, need) in str(ei.value) and "call again" in str(ei.value)
        for k in ("nbr_off", "top", "n_region"):
            assert np.array_equal(ei.value.out[k], want[k]), (cap, k)
    nm.check_equal(emu(tree, piv, 3, nm.TO, capacity=need), want, "exact capacity")
    # the same with a pass per pivot: the lists stop at the first pass that does not fit, the sizes go on
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("WEPP_NBR_PASS_COLS", "1")
        with pytest.raises(w.WeppError) as ei:
            emu(tree, piv, 3, nm.TO, capacity=need - 1)
        assert ei.value.code == 4
        for k in ("nbr_off", "top", "n_region"):
            assert np.array_equal(ei.value.out[k], want[k]), k
        nm.check_equal(emu(tree, piv, 3, nm.TO, capacity=need), want, "exact capacity, passes")
    # argument errors
    for bad, form, what in ((np.zeros(0, np.uint32), nm.TO, "null argument"), ([0, ar.n], nm.TO, "piv[1] = %d is not an arena index of this tree (%d haplotypes)" % (ar.n, ar.n)),
                            ([1, 0, 1], nm.TO, "haplotype 1 is a pivot more than once"), ([0], 2, "unknown form 2"), ([0], -1, "unknown form -1")):
        with pytest.raises(w.WeppError) as ei:
            emu(tree, bad, 1, form)
        assert ei.value.code == 1 and what in str(ei.value), bad
        if len(bad):
            with pytest.raises(w.WeppError) as ei:
                epp_emu.distances(tree, bad, form)
            assert ei.value.code == 1 and what in str(ei.value), bad
