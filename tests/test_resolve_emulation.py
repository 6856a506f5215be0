"""The kernels of wepp_epp_resolve without a GPU: resolve_kernels.hip (and assign_kernels.hip, which runs between its
mark and tally passes) compiled as plain C++ against tests/cxx/hip_emu -- one host thread per lane, lock step at every
cross-lane operation -- and driven as resolve_capi.cpp drives them, against the sequential model
(tests/resolve_model.py).  A relation list is cut into chunks of RES_CHUNK = 256 reads (resolve.hpp); lists of 255,
256 and 257 reads are covered below.  The device itself is the business of tests/test_epp_resolve_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import epp_fuzz
import fuzz_trees as ft
import resolve_cases as rc
import resolve_model as rm
import wepp_amd as w

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
RES_CHUNK = 256


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("resolve_emu") / "libresolve_emu.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-w", "-I", os.path.join(CXX, "resolve_emu_inc"),
                           "-I", os.path.join(CXX, "hip_emu"), os.path.join(CXX, "resolve_emu.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_resolve.restype = ctypes.c_longlong
    lib.emu_res_chunk.restype = ctypes.c_uint32
    assert lib.emu_res_chunk() == RES_CHUNK

    def run(tree, reads, genome, sel, residual):
        fv = w.FlatView(tree)
        woff, words, par = fv.get("node_woff"), fv.get("words"), fv.get("parent_dfs")
        words = words if words.size else np.zeros(1, np.uint32)
        max_pos = max(int(fv.get("maxnest").size), 1) - 1
        fv.close()
        R, K = reads.n_reads, len(sel)
        sel = np.ascontiguousarray(sel, np.uint32)
        res = np.array([int(w.pack_read_word(p, r, m)) for p, r, m in residual], np.uint32)
        M = int(res.size)
        order = np.lexsort((np.arange(R), reads.end, reads.start)).astype(np.uint32)      # (start, end, index)
        roff = np.zeros(M + 1, np.uint64); rrel = np.zeros(R * M + 1, np.uint32)
        ncov = np.zeros(M + 1, np.uint32); nmask = np.zeros(M + 1, np.uint32); bdeg = np.zeros(M + 1, np.int64)
        bmask = np.zeros((M, (K + 31) // 32), np.uint32)
        hr = np.zeros((M, K), np.uint32); hd = np.zeros((M, K), np.int64); nt = np.zeros(1, np.uint32)
        rw = reads.read_word if reads.read_word.size else np.zeros(1, np.uint32)
        resp = res if M else np.zeros(1, np.uint32)
        n = lib.emu_resolve(P(woff), P(words), P(par), max_pos, R, P(reads.read_off), P(rw), P(reads.start), P(reads.end),
                            P(reads.degree), P(order), genome, K, P(sel), M, P(resp), P(roff), P(rrel), P(ncov), P(nmask),
                            P(bdeg), P(bmask if bmask.size else np.zeros(1, np.uint32)), P(hr if hr.size else np.zeros(1, np.uint32)),
                            P(hd if hd.size else np.zeros(1, np.int64)), P(nt))
        assert n >= 0, n
        assert n == int(roff[M])
        bits = np.unpackbits(bmask.view(np.uint8), axis=1, bitorder="little")[:, :K] if M else np.zeros((0, K), np.uint8)
        return dict(rel_off=roff, rel_read=rrel[:n], n_covered=ncov[:M], n_masked=nmask[:M], best_degree=bdeg[:M], best_mask=bmask,
                    best=[np.flatnonzero(b).astype(np.uint32) for b in bits], hap_reads=hr, hap_degree=hd, n_touched=int(nt[0]))
    return run


HAND = rc.hand_cases()


@pytest.mark.parametrize("i", range(len(HAND)), ids=[c[0].replace(" ", "") for c in HAND])
def test_hand_cases(emu, i):
    name, tree, reads, genome, sel, residual = HAND[i]
    rm.check_equal(emu(tree, reads, genome, sel, residual), rm.resolve(tree, reads, genome, sel, residual), name)


def test_fuzz_trees(emu):
    rng = np.random.default_rng(8)
    total = dict.fromkeys(rm.BRANCHES, 0)
    for it in range(8):
        tree, ref = ft.random_tree(rng, genome=60)
        reads = epp_fuzz.random_epp_reads(rng, tree, ref, 60, n_reads=int(rng.integers(1, 25)))
        n = tree.n_nodes
        K = min(n, [1, 2, 3, 5, 63, 64, 65, n][it])
        sel = rng.permutation(n)[:K].astype(np.uint32)
        residual = rc.draw_residual(rng, reads, ref, 60, int(rng.integers(1, 13)))
        want = rm.resolve(tree, reads, 60, sel, residual)
        for k, v in want["branches"].items():
            total[k] += v
        rm.check_equal(emu(tree, reads, 60, sel, residual), want, (it, K))
    assert all(v > 0 for v in total.values()), total


# both sides of a best_mask word pair (64 columns per ballot) and of a slab (256 columns per pass of the tally)
@pytest.mark.parametrize("K", [1, 64, 65, 256, 257])
def test_selection_sizes(emu, K):
    g = w.generate_tree(11, 600, genome_len=3000)
    reads = g.reads(12, 10, read_len=150, p_substitution=0.003, p_n=0.02, windows=True, max_degree=5)
    sel = np.random.default_rng(K).permutation(600)[:K].astype(np.uint32)
    residual = rc.draw_residual(np.random.default_rng(K + 1), reads, rc.reference_of(g, reads), 3000, 12)
    want = rm.resolve(g.tree, reads, 3000, sel, residual)
    assert want["n_touched"] > 0
    rm.check_equal(emu(g.tree, reads, 3000, sel, residual), want, K)


def test_empty_residual_list(emu):
    _, tree, reads, genome, sel, _ = HAND[0]
    got = emu(tree, reads, genome, sel, [])
    assert got["n_touched"] == 0 and got["rel_off"].tolist() == [0] and got["rel_read"].size == 0


@pytest.mark.parametrize("n_reads", [RES_CHUNK - 1, RES_CHUNK, RES_CHUNK + 1])
def test_relation_list_around_a_chunk(emu, n_reads):
    tree, reads, genome, sel, residual = rc.long_list_case(n_reads)
    want = rm.resolve(tree, reads, genome, sel, residual)
    assert int(want["n_covered"][1]) == n_reads and int(want["n_covered"][0]) == 0
    rm.check_equal(emu(tree, reads, genome, sel, residual), want, n_reads)
