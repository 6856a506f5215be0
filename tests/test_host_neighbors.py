"""`wepp-epp --neighbors FILE [--radius R] [--max-neighbors L]`: haplotype_neighbors.csv and next_selection.txt
(arena::closest_neighbors, src/WEPP/arena.cpp:171-207, and the "add neighbors" step of post_filter.hpp:56-64) on the
fixture of test_host_wepp.py, against the literal model (tests/neighbors_model.py) ranked by the reference's
score_comparator (arena.hpp:16-30) over the oracle's scores and the leaf counts of the uncondensed tree."""
import functools
import subprocess

import numpy as np
import pytest

import neighbors_model as nm
import wepp_amd as w
from test_host_wepp import CLI, _as_reads, _condense, _setup, _sites

pytestmark = pytest.mark.gpu

SCORE_EPSILON = 1e-9


def _leaves_below(parent, node):
    kids = [[] for _ in parent]
    for i, p in enumerate(parent):
        if p >= 0:
            kids[p].append(i)
    n, todo = 0, [node]
    while todo:
        x = todo.pop()
        n += not kids[x]
        todo += kids[x]
    return n


def test_neighbor_files(tmp_path, oracle):
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
    full = m["score"] * np.sqrt(m["divergence"])                # haplotype::full_score
    leaves = [_leaves_below(parent, csrc[i][0]) for i in dfs_ids]   # get_num_leaves: below the first source node
    # the epsilon comparator is a strict weak order here: scores are equal or far apart
    gap = np.abs(full[:, None] - full[None, :])
    assert not np.isnan(full).any() and not ((gap > 1e-12) & (gap <= 1e-6)).any()
    assert (gap[np.triu_indices(n, 1)] <= 1e-12).any() and len(set(leaves)) > 2

    def cmp(a, b):
        if abs(full[a] - full[b]) > SCORE_EPSILON:
            return -1 if full[a] > full[b] else 1
        if leaves[a] != leaves[b]:
            return -1 if leaves[a] > leaves[b] else 1
        return -1 if ids[a] > ids[b] else (1 if ids[a] < ids[b] else 0)
    key = functools.cmp_to_key(cmp)

    ar = nm.Arena(ctree)
    K = 17
    sel = [int(k) for k in rng.permutation(n)[:K]]
    sel_file = tmp_path / "selected.txt"
    sel_file.write_text("".join(ids[k] + ("\t0.25\n", ",x,y\n", "\n")[j % 3] for j, k in enumerate(sel)))
    base = [CLI, "-i", pb, "-r", rpb, "-f", fa, "-m", bed]
    truncated = 0
    for extra, radius, limit in (([], 2, 500), (["--radius", "3", "--max-neighbors", "4"], 3, 4), (["--radius", "0"], 0, 500)):
        out = tmp_path / ("out_%d_%d" % (radius, limit))
        out.mkdir()
        r = subprocess.run(base + ["-d", str(out), "--neighbors", str(sel_file)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        rows, union = [], set()
        for p in sel:
            reg = ar.closest_neighbors(p, radius)
            truncated += len(reg) > limit
            ranked = sorted(reg, key=key)[:limit]
            union |= set(ranked)
            rows.append(",".join([ids[p]] + ["%s:%d" % (ids[h], reg[h]) for h in ranked]))
        assert (out / "haplotype_neighbors.csv").read_text().splitlines() == rows
        assert (out / "next_selection.txt").read_text().splitlines() == [ids[h] for h in sorted(union, key=key)]
        if radius == 2:
            assert any(len(row.split(",")) > 3 for row in rows) and len(union) > K
        # the map's files are written as before
        assert (out / "haplotype_scores.tsv").exists() and (out / "read_placements.tsv").exists()
    assert truncated > 0
    # the next selection is a selection: --assign reads it
    out = tmp_path / "again"
    out.mkdir()
    r = subprocess.run(base + ["-d", str(out), "--assign", str(tmp_path / "out_2_500" / "next_selection.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and (out / "haplotype_coverage.csv").exists(), r.stderr
    # an unknown identifier and bad options are errors
    sel_file.write_text(ids[sel[0]] + "\nno_such_haplotype\n")
    r = subprocess.run(base + ["-d", str(out), "--neighbors", str(sel_file)], capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR" in r.stderr
    sel_file.write_text(ids[sel[0]] + "\n")
    for extra in (["--radius", "-1"], ["--max-neighbors", "0"]):
        r = subprocess.run(base + ["-d", str(out), "--neighbors", str(sel_file)] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stderr
