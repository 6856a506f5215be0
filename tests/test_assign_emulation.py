"""wepp_epp_assign without a GPU: the entry point's own host code (assign_capi.cpp, epp_host.cpp) on assign_kernels.hip
compiled as plain C++ and an emulated HIP runtime (tests/epp_emu.py, tests/cxx/hip_emu: one host thread per lane, lock
step at every cross-lane operation), against the NumPy model.  Checks the host side's and the kernels' logic, sizes and
indexing; the device itself, and the largest layout unit, are the business of tests/test_epp_assign_gpu.py."""
import numpy as np
import pytest

import assign_model as am
import epp_emu
import epp_fuzz
import fuzz_trees as ft
import wepp_amd as w

emu = epp_emu.assign


def test_fuzz_trees():
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
def test_layout_edges(n_nodes, K, n_reads):
    g = w.generate_tree(11, n_nodes, genome_len=3000)
    reads = g.reads(12, n_reads, read_len=150, p_substitution=0.003, p_n=0.02, windows=True, max_degree=5)
    sel = np.random.default_rng(K).permutation(n_nodes)[:K].astype(np.uint32)
    am.check_equal(emu(g.tree, reads, 3000, sel), am.assign(g.tree, reads, 3000, sel), K)


def test_more_than_127_window_entries():
    """the byte counters of a lane are flushed every 127 entries inside the window"""
    g = w.generate_tree(5, 2000, genome_len=3000)
    reads = g.reads(21, 6, read_len=1200, amplicon_len=1200, amplicon_step=1000, p_substitution=0.003, p_n=0.2, windows=True,
                    max_degree=3)
    assert int(np.diff(reads.read_off).max()) > 200
    sel = np.random.default_rng(3).permutation(2000)[:300].astype(np.uint32)
    am.check_equal(emu(g.tree, reads, 3000, sel), am.assign(g.tree, reads, 3000, sel), "long")


OTHERS = ("min_dist", "n_epp", "asg_off", "sel_reads", "sel_degree", "sel_covered", "cover_bits")


def test_capacity_protocol_and_no_reads():
    rng = np.random.default_rng(4243)
    tree, ref = ft.random_tree(rng, genome=60, n_nodes=100)
    reads = epp_fuzz.random_epp_reads(rng, tree, ref, 60, n_reads=25)
    sel = rng.permutation(100)[:40].astype(np.uint32)
    want = am.assign(tree, reads, 60, sel)
    need = int(want["asg_off"][-1])
    assert need > 25
    for cap in (0, 1, need - 1):
        with pytest.raises(w.WeppError) as ei:
            emu(tree, reads, 60, sel, capacity=cap)
        assert ei.value.code == 4 and "asg_sel holds %d entries, %d needed" % (cap, need) in str(ei.value) and "call again" in str(ei.value)
        for k in OTHERS:
            assert np.array_equal(ei.value.out[k], want[k]), (cap, k)
    am.check_equal(emu(tree, reads, 60, sel, capacity=need), want, "exact capacity")
    # no reads: the per-haplotype outputs are zeroed on the host
    got = emu(tree, w.EppReads.from_lists([], [], []), 60, sel, capacity=4)
    assert got["asg_off"][0] == 0
    assert not got["sel_reads"].any() and not got["sel_degree"].any() and not got["sel_covered"].any() and not got["cover_bits"].any()
