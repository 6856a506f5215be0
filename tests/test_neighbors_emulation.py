"""The kernels of wepp_epp_neighbors without a GPU: neighbors_kernels.hip compiled as plain C++ against the HIP
stand-in (tests/cxx/hip_emu: one host thread per lane) and driven as neighbors_capi.cpp drives them, pass by pass,
against the literal model (tests/neighbors_model.py).  Checks the kernels' logic and indexing; the device is the
business of tests/test_epp_neighbors_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import neighbors_model as nm
import wepp_amd as w

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("neighbors_emu") / "libneighbors_emu.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-w", "-I", os.path.join(CXX, "hip_emu"),
                           os.path.join(CXX, "assign_emu.cpp"), os.path.join(CXX, "neighbors_emu.cpp"), "-o", so])
    lib = ctypes.CDLL(so)

    def run(tree, piv, radius, form, skip=None, pass_cols=None):
        fv = w.FlatView(tree)
        woff, words, par, end = fv.get("node_woff"), fv.get("words"), fv.get("parent_dfs"), fv.get("dfs_end") + 1
        words = words if words.size else np.zeros(1, np.uint32)
        max_pos = max(int(fv.get("maxnest").size), 1) - 1
        end = np.ascontiguousarray(end, np.uint32)
        fv.close()
        N, K = tree.n_nodes, len(piv)
        piv = np.ascontiguousarray(piv, np.uint32)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        off = np.zeros(K + 1, np.uint64); node = np.zeros(K * N, np.uint32); nd = np.zeros(K * N, np.int32)
        top = np.zeros(K, np.uint32); nreg = np.zeros(K, np.uint32); dist = np.zeros((K, N), np.int32)
        lib.emu_neighbors(P(woff), P(words), P(par), P(end), N, max_pos, K, P(piv), radius, form, P(sk) if sk is not None else None,
                          pass_cols or K, P(off), P(node), P(nd), P(top), P(nreg), P(dist))
        n = int(off[K])
        return dict(nbr_off=off, nbr_node=node[:n], nbr_dist=nd[:n], top=top, n_region=nreg), dist
    return run


def test_fuzz_trees(emu):
    for it, (tree, ar, piv) in enumerate(nm.fuzz_cases(10)):
        for form in (nm.TO, nm.FROM):
            for radius in (0, 2):
                got, dist = emu(tree, piv, radius, form)
                nm.check_equal(got, ar.neighbors(piv, radius, form), (it, form, radius))
            for i, p in enumerate(piv):
                assert np.array_equal(dist[i], ar.field(int(p), form)), (it, form, p)
        skip = (np.arange(ar.n) % 3 == 1).astype(np.uint8)
        nm.check_equal(emu(tree, piv, 2, nm.FROM, skip=skip)[0], ar.neighbors(piv, 2, nm.FROM, skip), (it, "skip"))
        nm.check_equal(emu(tree, piv, 1, nm.TO, pass_cols=1 + it % 3)[0], ar.neighbors(piv, 1, nm.TO), (it, "passes"))


@pytest.mark.parametrize("name", sorted(nm.hand_cases()))
def test_hand_cases(emu, name):
    tree, piv, radius, skip, _ = nm.hand_cases()[name]
    ar = nm.Arena(tree)
    for form in (nm.TO, nm.FROM):
        nm.check_equal(emu(tree, piv, radius, form, skip=skip)[0], ar.neighbors(piv, radius, form, skip), (name, form))


# both sides of the 256-row scan block, and more than 4 pivot columns in a pass; the 256-column slab is left to the GPU
@pytest.mark.parametrize("n_nodes", [255, 256, 257, 513])
def test_scan_block_edges(emu, n_nodes):
    g = w.generate_tree(11, n_nodes, genome_len=3000)
    ar = nm.Arena(g.tree)
    piv = np.array([0, n_nodes - 1, n_nodes // 2, 255 if n_nodes > 255 else 7, 254, 1], np.uint32)
    for form in (nm.TO, nm.FROM):
        got, dist = emu(g.tree, piv, 2, form)
        nm.check_equal(got, ar.neighbors(piv, 2, form), (n_nodes, form))
        assert np.array_equal(dist[1], ar.field(n_nodes - 1, form))


def test_chain_and_star(emu):
    A, C = w.A, w.C
    chain = w.Tree.from_lists([-1] + list(range(39)), [[(1 + i % 7, A, A if (i // 7) % 2 == 0 else C, C if (i // 7) % 2 == 0 else A)] for i in range(40)])
    star = w.Tree.from_lists([-1] + [0] * 39, [[]] + [[(1 + i % 5, A, A, C)] for i in range(39)])
    for tree in (chain, star):
        ar = nm.Arena(tree)
        piv = np.array([0, 39, 20], np.uint32)
        for form in (nm.TO, nm.FROM):
            for radius in (0, 1, 3):
                nm.check_equal(emu(tree, piv, radius, form)[0], ar.neighbors(piv, radius, form), (form, radius))
