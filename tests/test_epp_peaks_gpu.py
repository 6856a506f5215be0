"""wepp_epp_peaks on the GPU against the closed form of the model (tests/peaks_model.py, which test_peaks_model.py proves
equal to the line-by-line restatement of the reference).  Peaks, steps, tallies, removed reads and mapped flags are
integers: bit-exact.  score_left of an unmapped haplotype lies within the map's documented fixed-point bound of the
model's exact fraction and is exactly 0.0 where the model's is 0.  The map's outputs delivered by the call equal a
separate wepp_epp_map bit for bit.

Layout units whose two sides are covered (peaks.hpp, neighbors.hpp, epp_kernels.hip): a wave of 64 and a workgroup of
256 in the compaction of k_peak_hits and k_peak_ties, 256 haplotypes per workgroup of k_peak_max and per block of the
column scans, 2048 per workgroup of the score scan."""
import numpy as np
import pytest

import fuzz_trees as ft
import epp_fuzz
import peaks_model as pm
import wepp_amd as w

pytestmark = pytest.mark.gpu

EXACT = ("peaks", "peak_step", "peak_reads", "peak_degree", "removed_step", "removed_peak", "mapped")


def check_device(got, want, pb, tag=""):
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (tag, k, got[k], want[k])
    assert got["n_peaks"] == len(want["peaks"]), (tag, "n_peaks")
    assert got["n_steps"] == want["n_steps"] and got["n_remaining"] == want["n_remaining"], (tag, "counts", got["n_steps"], got["n_remaining"])
    bound = pm.score_bound(pb)
    for h in range(pb.N):
        if want["mapped"][h]:
            continue
        if want["score"][h] == 0:
            assert got["score_left"][h] == 0.0, (tag, "score_left is not exactly 0", h, got["score_left"][h])
        else:
            assert abs(got["score_left"][h] - float(want["score"][h])) <= bound[h] + 1e-15 * float(want["score"][h]), (tag, "score_left", h)


def check_map(got_map, mat, reads, genome, tag=""):
    sep = mat.epp_map(reads, genome)
    for k in ("max_parsimony", "multiplicity", "score", "counts", "divergence", "epp_off", "epp_nodes"):
        a, b = np.asarray(got_map[k]), np.asarray(sep[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, "map", k)


def run(mat, pb, par, **kw):
    return mat.epp_peaks(pb.reads, pb.genome, top_n=par[0], max_peaks=par[1], peak_radius=par[2], **kw)


@pytest.fixture(scope="module")
def fuzz():
    """the fuzz problems and the model's answers, computed once"""
    problems, closed = {}, {}
    for it, pb in pm.fuzz_problems():
        problems[it] = pb
        for par in pm.PARAMS:
            try:
                closed[it, par] = pm.peaks_closed(pb, *par)
            except pm.Ambiguous:
                closed[it, par] = None
    return problems, closed


@pytest.mark.parametrize("part", range(4))
def test_fuzz(fuzz, part):
    problems, closed = fuzz
    for it in sorted(problems):
        if it % 4 != part:
            continue
        pb = problems[it]
        mat = w.Mat(pb.tree)
        for par in pm.PARAMS:
            want = closed[it, par]
            if want is None:
                continue                                     # a near tie: fixed point and the model's fractions may part
            got = run(mat, pb, par, want_map=(par == pm.PARAMS[0]))
            check_device(got, want, pb, (it, par))
            if par == pm.PARAMS[0]:
                check_map(got["map"], mat, pb.reads, pb.genome, it)
        mat.close()


def test_fuzz_is_not_vacuous(fuzz):
    _, closed = fuzz
    busy = sum(1 for v in closed.values() if v is not None and v["n_steps"] > 1 and v["rejected"] > 0)
    assert busy * 3 >= len(closed)
    assert sum(1 for v in closed.values() if v is None) * 10 <= len(closed)


@pytest.mark.parametrize("name", sorted(pm.hand_cases()))
def test_hand_cases(name):
    tree, reads, par, exp = pm.hand_cases()[name]
    pb = pm.Problem(tree, reads, pm.GENOME)
    want = pm.peaks_closed(pb, *par)
    pm.check_expectations(want, exp, name)
    mat = w.Mat(tree)
    got = run(mat, pb, par, want_map=True)
    check_device(got, want, pb, name)
    if reads.n_reads:
        check_map(got["map"], mat, reads, pm.GENOME, name)
    else:
        assert (got["map"]["score"] == 0).all() and got["n_peaks"] == 0
    mat.close()


def _problem(seed, n_nodes, n_reads, tree_genome=pm.GENOME):
    rng = np.random.default_rng(seed)
    tree, ref = ft.random_tree(rng, n_nodes=n_nodes, genome=tree_genome, max_muts=2)
    ref = {p: ref.get(p, w.A) for p in range(0, pm.GENOME + 2)}
    reads = epp_fuzz.random_epp_reads(rng, tree, ref, pm.GENOME, n_reads=n_reads)
    return pm.Problem(tree, reads, pm.GENOME)


def _want(pb, par):
    """the model's answer for a layout case; the seeds below are chosen so that none is a near tie (Ambiguous fails)"""
    return pm.peaks_closed(pb, *par)


@pytest.mark.parametrize("n_reads", [63, 64, 65, 257])
def test_remaining_reads_at_wave_and_block_edges(n_reads):
    pb = _problem(100 + n_reads, 40, n_reads)
    mat = w.Mat(pb.tree)
    for par in ((10, 300, 1), (1, 300, 0)):
        check_device(run(mat, pb, par), _want(pb, par), pb, (n_reads, par))
    mat.close()


@pytest.mark.parametrize("n_nodes", [255, 256, 257, 513, 2049])
def test_nodes_at_block_edges(n_nodes):
    pb = _problem(200 + n_nodes, n_nodes, 48)
    assert pb.N == n_nodes
    mat = w.Mat(pb.tree)
    par = (10, 12, 1)
    check_device(run(mat, pb, par), _want(pb, par), pb, n_nodes)
    mat.close()


def test_subset_of_one_read_and_of_all_reads():
    A, C = w.A, w.C
    t2 = w.Tree.from_lists([-1, 0, 0], [[], [(10, A, A, C)], [(11, A, A, C)]])
    one_then_three = w.EppReads.from_lists([[(10, A, C)]] + [[(11, A, C)]] * 3, [10, 11, 11, 11], [10, 11, 12, 13], [9, 1, 1, 1])
    pb = pm.Problem(t2, one_then_three, pm.GENOME)
    want = pm.peaks_closed(pb, 10, 300, 0)
    assert [int(x) for x in want["peak_reads"]] == [1, 3] and want["n_steps"] == 2
    mat = w.Mat(t2)
    check_device(run(mat, pb, (10, 300, 0)), want, pb, "one then three")
    every = w.EppReads.from_lists([[]] * 70, [40] * 70, [45] * 70, [2] * 70)     # every read on every haplotype: one subset of all
    pb = pm.Problem(t2, every, pm.GENOME)
    want = pm.peaks_closed(pb, 1, 300, 0)
    assert [int(x) for x in want["peak_reads"]] == [70] and want["n_remaining"] == 0
    check_device(run(mat, pb, (1, 300, 0)), want, pb, "all")
    mat.close()


def test_tie_group_of_every_haplotype():
    """reads without entries in a window no mutation touches on a tree of 257 haplotypes: every score ties, the group is
    the whole tree (more than a workgroup of k_peak_ties), and the walk rejects what equals an accepted genotype"""
    rng = np.random.default_rng(77)
    tree, _ = ft.random_tree(rng, n_nodes=257, genome=30, max_muts=2)
    reads = w.EppReads.from_lists([[]] * 5, [40, 41, 42, 43, 44], [50, 51, 52, 53, 54], [1, 2, 3, 4, 5])
    pb = pm.Problem(tree, reads, pm.GENOME)
    assert all(m == 257 for m in pb.M)
    want = pm.peaks_closed(pb, 10, 300, 0)
    assert len(want["peaks"]) == 10 and want["n_steps"] == 1 and want["n_remaining"] == 0
    rank = np.arange(257, 0, -1).astype(np.uint32)           # ... and with ranks the walk starts at the other end
    want_r = pm.peaks_closed(pb, 10, 300, 0, tie_rank=rank)
    assert int(want_r["peaks"][0]) == 256
    mat = w.Mat(tree)
    check_device(run(mat, pb, (10, 300, 0)), want, pb, "all tie")
    check_device(run(mat, pb, (10, 300, 0), tie_rank=rank), want_r, pb, "all tie, ranks")
    mat.close()


def test_twice_on_one_handle_and_on_two_handles():
    pb = _problem(31, 120, 300)
    par = (10, 300, 1)
    want = pm.peaks_closed(pb, *par)
    assert want["n_steps"] > 1
    a, b = w.Mat(pb.tree), w.Mat(pb.tree)
    first = run(a, pb, par)
    check_device(first, want, pb, "first")
    t = w.epp_peaks_last_timing()
    assert t["map_ms"] > 0 and t["select_ms"] > 0 and t["hits_ms"] > 0 and t["remove_ms"] > 0 and t["clear_ms"] > 0
    for other in (run(a, pb, par), run(b, pb, par)):
        for k in EXACT + ("peak_score", "score_left"):
            assert np.asarray(other[k]).tobytes() == np.asarray(first[k]).tobytes(), k
        assert (other["n_steps"], other["n_remaining"]) == (first["n_steps"], first["n_remaining"])
    a.close(); b.close()


def test_arguments():
    A, C = w.A, w.C
    t2 = w.Tree.from_lists([-1, 0, 0], [[], [(10, A, A, C)], [(11, A, A, C)]])
    reads = w.EppReads.from_lists([[(10, A, C)]], [10], [10], [1])
    mat = w.Mat(t2)
    for kw in (dict(top_n=0), dict(max_peaks=0)):
        with pytest.raises(w.WeppError) as e:
            mat.epp_peaks(reads, 60, **kw)
        assert e.value.code == 1
    with pytest.raises(w.WeppError) as e:
        mat.epp_peaks(reads, 49)                             # the map's 50-bin rule
    assert e.value.code == 1
    empty = w.EppReads.from_lists([], [], [])
    got = mat.epp_peaks(empty, 60)
    assert got["n_peaks"] == 0 and got["n_steps"] == 0 and got["n_remaining"] == 0 and not got["mapped"].any()
    mat.close()
