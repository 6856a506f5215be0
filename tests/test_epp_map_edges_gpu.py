"""wepp_epp_map at the edges its fuzz never reaches at 64 nodes: streams cut into chunks, groups of several tiles,
the selection's scan carry and group skip, the list cap at equality, the reads-per-lane switch, the LDS limit and the
fixed-point scores against exact rational sums.  Inputs and the model come from tests/epp_cases.py; every test first
asserts, on the model and the oracle alone, that its input shows the edge (tests/test_epp_cases.py does the same on the
CPU), then compares the library with the oracle by the rules of tests/test_epp_gpu.py: integer outputs bit-exact,
scores within 1e-9 * (1 + |score|) of the oracle's double sum -- and, where the exact sums are cheap, within the bound
that follows from the library's own arithmetic (epp_cases.score_bound)."""
import functools
import time
from fractions import Fraction

import numpy as np
import pytest

import epp_cases as ec
import wepp_amd as w
from test_epp_gpu import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    monkeypatch.delenv("WEPP_EPP_RPL", raising=False)


def _check_exact(got, want, reads, n_nodes, tag):
    """Scores against the exact rational sums built from the oracle's integer outputs, counts against the oracle's and
    against the integer sum of the contributing reads' degrees."""
    exact, n_contrib, deg_sum = ec.exact_scores(want, reads.degree, n_nodes)
    total = int(reads.degree.astype(np.int64).sum())
    worst = Fraction(0)
    bad = []
    for n in range(n_nodes):
        err = abs(Fraction(float(got["score"][n])) - exact[n])
        bound = ec.score_bound(exact[n], n_contrib[n], total)
        if n_contrib[n]:
            worst = max(worst, err / bound)
        if err > bound:
            bad.append((n, float(err), float(bound)))
    print("%s: total degree %d, k = %d, worst |got - exact| / bound = %.3f" % (tag, total, ec.fx_bits(total), float(worst)))
    assert not bad, (tag, bad[:5])
    assert ((got["score"] == 0) == (n_contrib == 0)).all(), tag
    assert (got["counts"] == want["counts"]).all(), tag
    assert (got["counts"].astype(np.int64).sum(axis=1) == deg_sum).all(), tag


# ---- A. chunk cuts --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chunk_case(name, oracle):
    case = ec.chunk_case(name)
    return case, oracle.OracleTree(case["tree"]).epp_map(case["reads"], genome_size=case["genome"])


@pytest.mark.parametrize("rpl", [1, 4])
@pytest.mark.parametrize("name", sorted(ec.CHUNK_CASES))
def test_chunk_cuts(oracle, name, rpl, monkeypatch):
    """Window streams of 1024 / 1026 / 2048 / 2050 events: k_epp_combine stitches a read's minimum, multiplicity and
    list cursor over the pieces, pass 2 closes ranges at a piece's end and opens them again in the next job."""
    case, want = _chunk_case(name, oracle)
    shows, pl, gs = ec.chunk_edges(case, want, rpl)
    assert shows == ec.CHUNK_SHOWS[name]
    monkeypatch.setenv("WEPP_EPP_RPL", str(rpl))
    mat = w.Mat(case["tree"])
    got = mat.epp_map(case["reads"], case["genome"])
    t = w.epp_last_timing()
    mat.close()
    assert (t["groups"], t["jobs"]) == (pl["G"], ec.jobs(pl, gs))      # the cuts the model states are the cuts that ran
    _check(got, want, case["reads"].n_reads, (name, rpl))
    _check_exact(got, want, case["reads"], case["tree"].n_nodes, (name, rpl))


# ---- B. groups of several tiles -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reads", sorted(ec.GROUP_CASES))
def test_groups_of_several_tiles(oracle, n_reads, monkeypatch):
    """More than 512 tiles: a group's stream is wider than a tile's window, so the events of a run of 64 that lie in
    the tile are packed to the low lanes around holes, runs with none are skipped, and the jobs of a group are
    numbered chunk * ntiles + tile with ntiles > 1."""
    rpl, tpg, G, last = ec.GROUP_CASES[n_reads]
    case = ec.group_case(n_reads)
    e = ec.group_edges(case)
    pl = e["plan"]
    assert (pl["rpl"], pl["tpg"], pl["G"], int(pl["group_ntiles"][-1])) == (rpl, tpg, G, last)
    assert e["found"] is not None and e["n_holes"] > 100 and e["n_empty"] >= 1
    monkeypatch.setenv("WEPP_EPP_RPL", str(rpl))
    t0 = time.time()
    mat = w.Mat(case["tree"])
    got = mat.epp_map(case["reads"], case["genome"])
    t = w.epp_last_timing()
    mat.close()
    t1 = time.time()
    want = oracle.OracleTree(case["tree"]).epp_map(case["reads"], genome_size=case["genome"], nthreads=16)
    print("%d reads: library %.2f s, oracle %.2f s" % (n_reads, t1 - t0, time.time() - t1))
    assert (t["groups"], t["jobs"]) == (G, ec.jobs(pl, e["streams"]))
    _check(got, want, n_reads, n_reads)


# ---- C. selection ---------------------------------------------------------------------------------------------------
def test_selection_skips_groups(oracle):
    """An early long read: group 0 covers positions that the groups after it do not, so an event's next group is found
    by skipping those that end before it (k_epp_select_scatter)."""
    case = ec.group_skip_case()
    e = ec.skip_edges(case)
    pl = e["plan"]
    assert pl["G"] == 6 and pl["order"][0] == case["long_read"] and pl["group_we"][0] > pl["group_we"][1]
    assert e["found"] is not None and e["found"]["later"] >= 2
    mat = w.Mat(case["tree"])
    got = mat.epp_map(case["reads"], case["genome"])
    t = w.epp_last_timing()
    mat.close()
    assert t["groups"] == 6
    want = oracle.OracleTree(case["tree"]).epp_map(case["reads"], genome_size=case["genome"])
    _check(got, want, case["reads"].n_reads, "group skip")
    _check_exact(got, want, case["reads"], case["tree"].n_nodes, "group skip")


def test_select_scan_carry(oracle):
    """More than 256 selection blocks: k_epp_select_scan carries the running count from one round of 256 to the next."""
    case = ec.select_scan_case()
    assert int((case["tree"].mut_pos >= 0).sum()) > 131072 and ec.select_blocks(case["tree"]) > ec.SEL_SCAN_WIDTH
    reads = case["reads"]
    mat = w.Mat(case["tree"])
    got = mat.epp_map(reads, case["genome"])
    t = w.epp_last_timing()
    mat.close()
    want = oracle.OracleTree(case["tree"]).epp_map(reads, genome_size=case["genome"], nthreads=16)
    case["gen"].close()
    assert t["stream_events"] > 0
    _check(got, want, reads.n_reads, "select scan")


# ---- D. list cap ----------------------------------------------------------------------------------------------------
def test_list_cap_at_equality(oracle):
    """multiplicity <= max_cached_epp with reads of multiplicity 1, 2 and n_nodes interleaved in one tile."""
    case = ec.list_cap_case()
    reads, n = case["reads"], case["tree"].n_nodes
    want = oracle.OracleTree(case["tree"]).epp_map(reads, genome_size=case["genome"])
    assert (want["multiplicity"] == case["kind"]).all() and set(case["kind"].tolist()) == {1, 2, n}
    assert case["caps"] == (0, 1, n - 1, n, n + 1)
    mat = w.Mat(case["tree"])
    kept_sets = []
    for cap in case["caps"]:
        cut, keep = ec.cut_lists(want, cap)
        kept_sets.append(tuple(keep.tolist()))
        got = mat.epp_map(reads, case["genome"], max_cached_epp=cap)
        assert (got["epp_off"] == cut["epp_off"]).all() and (got["epp_nodes"] == cut["epp_nodes"]).all(), cap
        _check(got, cut, reads.n_reads, cap)
    mat.close()
    assert len(set(kept_sets[:4])) == 4 and kept_sets[4] == kept_sets[3]


# ---- E. exact scores ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ec.SCORE_BATCHES)
@pytest.mark.parametrize("which", sorted(ec.DEGREE_TOTALS))
def test_scores_within_the_fixed_point_bound(oracle, which, batch):
    """Total degrees of 2^10 - 1, 2^10 and 2^31 - 1: 52, 51 and 31 bits behind the binary point.  The `sparse` batch
    gives every haplotype one read, so that a single wrong rounding exceeds the bound."""
    case = ec.score_case(which, batch)
    reads, tree = case["reads"], case["tree"]
    total = int(reads.degree.astype(np.int64).sum())
    assert total == ec.DEGREE_TOTALS[which] and ec.fx_bits(total) == {"k52": 52, "k51": 51, "k31": 31}[which]
    want = oracle.OracleTree(tree).epp_map(reads, genome_size=case["genome"])
    mat = w.Mat(tree)
    got = mat.epp_map(reads, case["genome"])
    mat.close()
    _check(got, want, reads.n_reads, (which, batch))
    _check_exact(got, want, reads, tree.n_nodes, (which, batch))


# ---- F. reads per lane, LDS limit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("longest,rpl,groups", [(383, 4, 2), (384, 1, 5)])
def test_reads_per_lane_switch(oracle, longest, rpl, groups, monkeypatch):
    """WEPP_EPP_RPL=4 holds up to a longest read of 383 (tiles of 256 reads) and falls back to 1 from 384 on."""
    case = ec.rpl_switch_case(longest)
    reads = case["reads"]
    assert reads.n_reads == 300 and ec.effective_rpl(reads.start, reads.end, 4) == rpl
    assert ec.plan(reads.start, reads.end, rpl)["G"] == groups
    monkeypatch.setenv("WEPP_EPP_RPL", "4")
    mat = w.Mat(case["tree"])
    got = mat.epp_map(reads, case["genome"])
    t = w.epp_last_timing()
    mat.close()
    assert t["groups"] == groups
    want = oracle.OracleTree(case["tree"]).epp_map(reads, genome_size=case["genome"])
    _check(got, want, reads.n_reads, longest)
    _check_exact(got, want, reads, case["tree"].n_nodes, longest)


def test_lds_limit(oracle):
    """The longest read whose tile fits 150 KiB of LDS is placed; one position more is WEPP_ELIMIT "reads too long",
    and the handle goes on working."""
    below, above = ec.lds_limit_spans()
    assert ec.lds_bytes(below) <= 150 * 1024 < ec.lds_bytes(above)
    case = ec.lds_limit_case(below)
    mat = w.Mat(case["tree"])
    got = mat.epp_map(case["reads"], case["genome"])
    want = oracle.OracleTree(case["tree"]).epp_map(case["reads"], genome_size=case["genome"])
    _check(got, want, 1, "below the limit")
    over = ec.lds_limit_case(above)
    with pytest.raises(w._lib.WeppError) as err:
        mat.epp_map(over["reads"], over["genome"])
    assert err.value.code == 4 and "reads too long" in str(err.value)
    got = mat.epp_map(case["ordinary"], case["genome"])
    want = oracle.OracleTree(case["tree"]).epp_map(case["ordinary"], genome_size=case["genome"])
    _check(got, want, case["ordinary"].n_reads, "after the error")
    mat.close()
