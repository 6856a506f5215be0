"""The sorted pass of place_dev.hpp without a GPU: sorted_fill / sorted_build / sorted_query compiled as plain C++
against tests/cxx/hip_emu (one host thread per lane, in lock step at every barrier) and run by a workgroup of two waves
(k_step) and of four (k_walk_wave) against the all-pairs definition (sorted_pass_model.py).  The reads of a launch go
through ONE workgroup one after the other, sizes mixed, so a read also meets what the read before it left in LDS."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sorted_pass_model as spm

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sorted_pass_emu") / "libsorted_pass_emu.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-w", "-I", os.path.join(CXX, "hip_emu"),
                           os.path.join(CXX, "sorted_pass_emu.cpp"), "-o", so])
    lib = ctypes.CDLL(so)

    def run(waves, reads):
        n = len(reads)
        node = np.full((n, 256), spm.NONE, np.uint32); end = np.full((n, 256), spm.NONE, np.uint32)
        pk = np.zeros((n, 256), np.uint32); E = np.array([len(r) for r in reads], np.uint32)
        for i, r in enumerate(reads):
            node[i, :len(r)], end[i, :len(r)], pk[i, :len(r)] = [e[0] for e in r], [e[1] for e in r], [e[2] for e in r]
        out = np.zeros((n, 256, 6), np.uint32)
        assert lib.emu_sorted_pass(waves, P(node), P(end), P(pk), P(E), n, P(out)) == 0
        # (cb, cB are signed)
        return [[tuple(int(np.int32(v)) if f < 2 else int(v) for f, v in enumerate(out[i, j])) for j in range(len(r))] for i, r in enumerate(reads)]
    return run


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(11)
    named = spm.hand_made(rng)
    # large and small reads in turn behind them: 256 / 65 / 129 / 193 entries
    for rep in range(3):
        for E in (256, 65, 129, 193):
            named.append((f"in turn {rep}, E={E}", spm.random_tree_entries(rng, E, 40 + 30 * rep)))
    return named, [spm.all_pairs(e) for _, e in named]


@pytest.mark.parametrize("waves", [2, 4])
def test_lanes_against_all_pairs(emu, cases, waves):
    named, want = cases
    got = emu(waves, [e for _, e in named])
    for (name, _), g, x in zip(named, got, want):
        spm.assert_same(g, x, f"{waves} waves, {name}")
