"""The kernels of wepp_epp_assign without a GPU: assign_kernels.hip compiled as plain C++ against a stand-in for the
HIP pieces it uses (tests/cxx/hip_emu: one host thread per lane, lock step at every cross-lane operation) and driven
as assign_capi.cpp drives them, against the NumPy model.  Checks the kernels' logic and indexing; the device itself, and the largest layout unit, are the
business of tests/test_epp_assign_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assign_model as am
import epp_fuzz
import fuzz_trees as ft
import wepp_amd as w

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("assign_emu") / "libassign_emu.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-w", "-I", os.path.join(CXX, "hip_emu"),
                           os.path.join(CXX, "assign_emu.cpp"), "-o", so])
    lib = ctypes.CDLL(so)

    def run(tree, reads, genome, sel):
        fv = w.FlatView(tree)
        woff, words, par = fv.get("node_woff"), fv.get("words"), fv.get("parent_dfs")
        words = words if words.size else np.zeros(1, np.uint32)
        max_pos = max(int(fv.get("maxnest").size), 1) - 1
        fv.close()
        R, K = reads.n_reads, len(sel)
        sel = np.ascontiguousarray(sel, np.uint32)
        order = np.lexsort((np.arange(R), reads.end, reads.start)).astype(np.uint32)      # (start, end, index)
        md = np.zeros(R, np.int32); ne = np.zeros(R, np.uint32); off = np.zeros(R + 1, np.uint64)
        asel = np.zeros(R * K + 1, np.uint32); sr = np.zeros(K, np.uint32); sd = np.zeros(K, np.int64); sc = np.zeros(K, np.uint32)
        cover = np.zeros((K, (genome + 31) // 32), np.uint32)
        rw = reads.read_word if reads.read_word.size else np.zeros(1, np.uint32)
        lib.emu_assign(P(woff), P(words), P(par), max_pos, R, P(reads.read_off), P(rw), P(reads.start), P(reads.end),
                       P(reads.degree), P(order), genome, K, P(sel), P(md), P(ne), P(off), P(asel), P(sr), P(sd), P(sc), P(cover))
        return dict(min_dist=md, n_epp=ne, asg_off=off, asg_sel=asel[:int(off[R])], sel_reads=sr, sel_degree=sd,
                    sel_covered=sc, cover_bits=cover)
    return run


def test_fuzz_trees(emu):
    rng = np.random.default_rng(5)
    for it in range(9):
        tree, ref = ft.random_tree(rng, genome=60)
        reads = epp_fuzz.random_epp_reads(rng, tree, ref, 60, n_reads=int(rng.integers(1, 25)))
        n = tree.n_nodes
        K = min(n, [1, 2, 3, 4, 5, 63, 64, 65, n][it])
        sel = rng.permutation(n)[:K].astype(np.uint32)
        am.check_equal(emu(tree, reads, 60, sel), am.assign(tree, reads, 60, sel), (it, K))


# both sides of a slab (256) and of the register-resident group (1 024).  The LDS counters' limit (5 120 columns) takes
# half a minute per side here -- a host barrier per emulated workgroup -- and is left to the GPU test.
@pytest.mark.parametrize("n_nodes,K,n_reads", [(600, 256, 8), (600, 257, 8), (1100, 1024, 6), (1100, 1025, 6)])
def test_layout_edges(emu, n_nodes, K, n_reads):
    g = w.generate_tree(11, n_nodes, genome_len=3000)
    reads = g.reads(12, n_reads, read_len=150, p_substitution=0.003, p_n=0.02, windows=True, max_degree=5)
    sel = np.random.default_rng(K).permutation(n_nodes)[:K].astype(np.uint32)
    am.check_equal(emu(g.tree, reads, 3000, sel), am.assign(g.tree, reads, 3000, sel), K)


def test_more_than_127_window_entries(emu):
    """the byte counters of a lane are flushed every 127 entries inside the window"""
    g = w.generate_tree(5, 2000, genome_len=3000)
    reads = g.reads(21, 6, read_len=1200, amplicon_len=1200, amplicon_step=1000, p_substitution=0.003, p_n=0.2, windows=True,
                    max_degree=3)
    assert int(np.diff(reads.read_off).max()) > 200
    sel = np.random.default_rng(3).permutation(2000)[:300].astype(np.uint32)
    am.check_equal(emu(g.tree, reads, 3000, sel), am.assign(g.tree, reads, 3000, sel), "long")
