"""`wepp-epp --peaks [--top-n --max-peaks --peak-radius]`: the whole of wepp_filter::filter (src/WEPP/initial_filter.cpp:
455-506) on the fixture of test_host_wepp.py.  peaks.txt equals the model's peaks (tests/peaks_model.py, the closed form
with tie ranks from the leaf counts of the uncondensed tree and the identifiers) plus the model's expansion (the regions
of tests/neighbors_model.py ranked by score_comparator over the oracle's original scores); peak_reads.csv equals the
model's tallies; and the file feeds --assign unchanged."""
import functools
import subprocess

import numpy as np
import pytest

import peaks_model as pm
import wepp_amd as w
from test_host_neighbors import SCORE_EPSILON, _leaves_below
from test_host_wepp import CLI, _as_reads, _condense, _setup, _sites

pytestmark = pytest.mark.gpu


def test_peak_files(tmp_path, oracle):
    rng = np.random.default_rng(78)
    mask = (15, 64)
    genome = 200
    tree, parent, muts, newname, reference, recs, pb, rpb, fa, bed = _setup(tmp_path, rng, 250, 400, genome=genome, mask=mask)
    ents, start, end, degree = _as_reads(recs, reference, mask)
    cpar, cmuts, csrc, corig = _condense(parent, [[(m[0], m[1], m[3]) for m in ml] for ml in muts], _sites(ents, start, end, mask))
    ctree = w.Tree.from_lists(cpar, cmuts)
    reads = w.EppReads.from_lists(ents, start, end, degree)
    ot = oracle.OracleTree(ctree)
    m = ot.epp_map(reads, genome_size=genome)
    dfs_ids = ot.dfs_ids()
    ot.close()
    n = len(dfs_ids)
    ids = [newname[corig[i]] for i in dfs_ids]                  # identifier of the haplotype with arena index k
    full = m["score"] * np.sqrt(m["divergence"])                # haplotype::full_score, original
    leaves = [_leaves_below(parent, csrc[i][0]) for i in dfs_ids]

    # score_comparator's last two criteria as the rank wepp_epp_peaks takes: more leaves first, then the larger identifier
    by_rank = sorted(range(n), key=functools.cmp_to_key(
        lambda a, b: (leaves[b] > leaves[a]) - (leaves[b] < leaves[a]) or (ids[b] > ids[a]) - (ids[b] < ids[a])))
    tie_rank = [0] * n
    for k, h in enumerate(by_rank):
        tie_rank[h] = k

    def cmp(a, b):                                              # arena.hpp:16-31 over the original scores
        if abs(full[a] - full[b]) > SCORE_EPSILON:
            return -1 if full[a] > full[b] else 1
        return -1 if tie_rank[a] < tie_rank[b] else (1 if tie_rank[a] > tie_rank[b] else 0)
    key = functools.cmp_to_key(cmp)

    prob = pm.Problem(ctree, reads, genome)
    assert np.allclose([float(x) for x in prob.score], m["score"], rtol=1e-12, atol=1e-12)      # the model's map is the oracle's
    base = [CLI, "-i", pb, "-r", rpb, "-f", fa, "-m", bed]
    busy = 0
    for extra, par in (([], (10, 300, 2)), (["--top-n", "3", "--max-peaks", "7", "--peak-radius", "1"], (3, 7, 1)),
                       (["--top-n", "1", "--peak-radius", "0"], (1, 300, 0))):
        want = pm.peaks_closed(prob, *par, tie_rank=tie_rank)   # (Ambiguous fails the test: the fixture's seed avoids near ties)
        peaks = [int(p) for p in want["peaks"]]
        nbrs, kept = pm.expansion(prob, set(peaks), key, par[2])
        out = tmp_path / ("out_%d_%d_%d" % par)
        out.mkdir()
        r = subprocess.run(base + ["-d", str(out), "--peaks"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert (out / "peaks.txt").read_text().split() == [str(h) for h in sorted(peaks) + nbrs], (par, r.stderr)
        rows = ["%s,%d,%d,%d" % (ids[p], want["peak_reads"][k], want["peak_degree"][k], want["peak_step"][k]) for k, p in enumerate(peaks)]
        assert (out / "peak_reads.csv").read_text().splitlines() == rows
        assert (out / "haplotype_scores.tsv").exists() and (out / "read_placements.tsv").exists()
        busy += want["n_steps"] > 1 and len(nbrs) > 0
        if par != (10, 300, 2):
            continue
        # the file feeds --assign as it is: the same selection as its identifiers name
        again, by_id = tmp_path / ("assign_%d_%d_%d" % par), tmp_path / ("assign_ids_%d_%d_%d" % par)
        again.mkdir(); by_id.mkdir()
        r = subprocess.run(base + ["-d", str(again), "--assign", str(out / "peaks.txt")], capture_output=True, text=True)
        assert r.returncode == 0 and (again / "haplotype_coverage.csv").exists(), r.stderr
        sel = tmp_path / "sel.txt"
        sel.write_text("".join(ids[h] + "\n" for h in sorted(peaks) + nbrs))
        r = subprocess.run(base + ["-d", str(by_id), "--assign", str(sel)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for name in ("haplotype_coverage.csv", "haplotype_reads.csv"):
            assert (again / name).read_text() == (by_id / name).read_text(), name
        assert [l.split(",")[0] for l in (again / "haplotype_coverage.csv").read_text().splitlines()] == [ids[h] for h in sorted(peaks) + nbrs]
    assert busy >= 2
    # bad options are errors
    for extra in (["--top-n", "0"], ["--max-peaks", "0"], ["--peak-radius", "-1"]):
        r = subprocess.run(base + ["-d", str(tmp_path), "--peaks"] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stderr
    # an index past the last haplotype is no selection
    sel = tmp_path / "bad.txt"
    sel.write_text("0\n%d\n" % n)
    r = subprocess.run(base + ["-d", str(tmp_path), "--assign", str(sel)], capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR" in r.stderr
