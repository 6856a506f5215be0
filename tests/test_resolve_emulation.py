"""wepp_epp_resolve without a GPU: the entry point's own host code (resolve_capi.cpp, epp_host.cpp) on
resolve_kernels.hip and assign_kernels.hip (which runs between the mark and tally passes) compiled as plain C++ and an
emulated HIP runtime (tests/epp_emu.py, tests/cxx/hip_emu: one host thread per lane, lock step at every cross-lane
operation), against the sequential model (tests/resolve_model.py).  A relation list is cut into chunks of
RES_CHUNK = 256 reads (resolve.hpp); lists of 255, 256 and 257 reads are covered below.  The device itself is the
business of tests/test_epp_resolve_gpu.py."""
import numpy as np
import pytest

import epp_emu
import epp_fuzz
import fuzz_trees as ft
import resolve_cases as rc
import resolve_model as rm
import wepp_amd as w

RES_CHUNK = 256
emu = epp_emu.resolve


def test_res_chunk():
    assert epp_emu.lib().emu_res_chunk() == RES_CHUNK


HAND = rc.hand_cases()


@pytest.mark.parametrize("i", range(len(HAND)), ids=[c[0].replace(" ", "") for c in HAND])
def test_hand_cases(i):
    name, tree, reads, genome, sel, residual = HAND[i]
    rm.check_equal(emu(tree, reads, genome, sel, residual), rm.resolve(tree, reads, genome, sel, residual), name)


def test_fuzz_trees():
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
def test_selection_sizes(K):
    g = w.generate_tree(11, 600, genome_len=3000)
    reads = g.reads(12, 10, read_len=150, p_substitution=0.003, p_n=0.02, windows=True, max_degree=5)
    sel = np.random.default_rng(K).permutation(600)[:K].astype(np.uint32)
    residual = rc.draw_residual(np.random.default_rng(K + 1), reads, rc.reference_of(g, reads), 3000, 12)
    want = rm.resolve(g.tree, reads, 3000, sel, residual)
    assert want["n_touched"] > 0
    rm.check_equal(emu(g.tree, reads, 3000, sel, residual), want, K)


def test_empty_residual_list():
    _, tree, reads, genome, sel, _ = HAND[0]
    got = emu(tree, reads, genome, sel, [])
    assert got["n_touched"] == 0 and got["rel_off"].tolist() == [0] and got["rel_read"].size == 0


@pytest.mark.parametrize("n_reads", [RES_CHUNK - 1, RES_CHUNK, RES_CHUNK + 1])
def test_relation_list_around_a_chunk(n_reads):
    tree, reads, genome, sel, residual = rc.long_list_case(n_reads)
    want = rm.resolve(tree, reads, genome, sel, residual)
    assert int(want["n_covered"][1]) == n_reads and int(want["n_covered"][0]) == 0
    rm.check_equal(emu(tree, reads, genome, sel, residual), want, n_reads)


def test_capacity_protocol_and_empty_inputs():
    rng = np.random.default_rng(4244)
    tree, ref = ft.random_tree(rng, genome=60, n_nodes=100)
    reads = epp_fuzz.random_epp_reads(rng, tree, ref, 60, n_reads=25)
    sel = rng.permutation(100)[:40].astype(np.uint32)
    residual = rc.draw_residual(rng, reads, ref, 60, 20)
    want = rm.resolve(tree, reads, 60, sel, residual)
    need = int(want["rel_off"][-1])
    assert need > 10
    for cap in (0, need - 1):
        with pytest.raises(w.WeppError) as ei:
            emu(tree, reads, 60, sel, residual, capacity=cap)
        assert ei.value.code == 4 and "rel_read holds %d entries, %d needed" % (cap, need) in str(ei.value) and "call again" in str(ei.value)
        for k in rm.KEYS:
            if k != "rel_read":
                assert np.array_equal(ei.value.out[k], want[k]), (cap, k)
        assert ei.value.out["n_touched"] == want["n_touched"]
    rm.check_equal(emu(tree, reads, 60, sel, residual, capacity=need), want, "exact capacity")
    # n_res == 0; no reads: the outputs are zeroed on the host
    got = emu(tree, reads, 60, sel, [], capacity=4)
    assert got["rel_off"].tolist() == [0] and got["n_touched"] == 0
    got = emu(tree, w.EppReads.from_lists([], [], []), 60, sel, residual, capacity=4)
    assert not got["rel_off"].any() and got["n_touched"] == 0
    for k in ("n_covered", "n_masked", "best_degree", "best_mask", "hap_reads", "hap_degree"):
        assert not got[k].any(), k


def test_no_touched_read():
    """the call returns after the mark's count pass: every output zeroed on the host"""
    name, tree, reads, genome, sel, residual = next(c for c in HAND if c[0].startswith("untouched"))
    got = emu(tree, reads, genome, sel, residual)
    assert got["n_touched"] == 0 and not got["rel_off"].any() and got["rel_read"].size == 0
    for k in ("n_covered", "n_masked", "best_degree", "best_mask", "hap_reads", "hap_degree"):
        assert not got[k].any(), k


def test_argument_errors():
    tree, ref = rc.hand_tree()
    reads = w.EppReads.from_lists([[(5, w.A, w.C)], []], [1, 10], [30, 40])
    for residual, what in (([(0, w.A, w.C)], "outside 1 .. genome_size"), ([(61, w.A, w.C)], "outside 1 .. genome_size"),
                           ([(5, w.A, 0)], "mut_nuc"), ([(5, w.A, 15)], "mut_nuc"), ([(5, w.A | w.C, w.C)], "one-hot"),
                           ([(5, 0, w.C)], "one-hot"), ([(5, w.A, w.C), (7, w.A, w.N)], "residual mutation 1")):
        with pytest.raises(w.WeppError) as ei:
            emu(tree, reads, 60, [0, 1], residual)
        assert ei.value.code == 1 and what in str(ei.value), residual
    # the checks of wepp_epp_assign, same codes and messages
    with pytest.raises(w.WeppError) as ei:
        emu(tree, reads, 60, [0, 4], [(5, w.A, w.C)])
    assert ei.value.code == 1 and "sel[1] = 4 is not an arena index of this tree (4 haplotypes)" in str(ei.value)
    with pytest.raises(w.WeppError) as ei:
        emu(tree, reads, 60, [1, 0, 1], [(5, w.A, w.C)])
    assert ei.value.code == 1 and "haplotype 1 is selected more than once" in str(ei.value)
    with pytest.raises(w.WeppError) as ei:
        emu(tree, reads, 0, [0], [(5, w.A, w.C)])
    assert ei.value.code == 1 and "genome_size" in str(ei.value)
    bad = w.EppReads.from_lists([[(3, w.A, w.A)]], [1], [10])
    with pytest.raises(w.WeppError) as ei:
        emu(tree, bad, 60, [0], [(5, w.A, w.C)])
    assert "must differ from the reference base" in str(ei.value)
