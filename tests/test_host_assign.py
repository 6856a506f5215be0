"""`wepp-epp --assign FILE`: haplotype_reads.csv and haplotype_coverage.csv (the files of
arena::dump_read2haplotype_mapping, src/WEPP/arena.cpp:590-696) on the fixture of test_host_wepp.py, against
the model of wepp_epp_assign (tests/assign_model.py)."""
import subprocess

import numpy as np
import pytest

import assign_model as am
import pb_fixture as pbf
import wepp_amd as w
from test_host_wepp import CLI, _as_reads, _condense, _setup, _sites

pytestmark = pytest.mark.gpu


def test_assign_files(tmp_path, oracle):
    rng = np.random.default_rng(78)
    mask = (15, 64)
    genome = 200
    tree, parent, muts, newname, reference, recs, pb, rpb, fa, bed = _setup(tmp_path, rng, 250, 400, genome=genome, mask=mask)
    # the column table of the reads file: a read stands for itself, for two merged reads, or (rarely) is not listed
    merge = {}
    for q, rec in enumerate(recs):
        if q % 7:
            merge[rec[0]] = [rec[0]] if q % 3 else [rec[0] + "_a", rec[0] + "_b"]
    pbf.write_reads_pb(rpb, recs, merge)
    ents, start, end, degree = _as_reads(recs, reference, mask)
    cpar, cmuts, csrc, corig = _condense(parent, [[(m[0], m[1], m[3]) for m in ml] for ml in muts], _sites(ents, start, end, mask))
    ctree = w.Tree.from_lists(cpar, cmuts)
    reads = w.EppReads.from_lists(ents, start, end, degree)
    ot = oracle.OracleTree(ctree)
    ids = [newname[corig[i]] for i in ot.dfs_ids()]              # identifier of the haplotype with arena index k
    ot.close()
    K = min(17, len(ids))
    sel = rng.permutation(len(ids))[:K]
    sel_file = tmp_path / "selected.txt"
    sel_file.write_text("".join(ids[k] + ("\t0.25\n", ",x,y\n", "\n")[j % 3] for j, k in enumerate(sel)) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    base = [CLI, "-i", pb, "-r", rpb, "-f", fa, "-m", bed, "-d", str(out)]
    r = subprocess.run(base + ["--assign", str(sel_file)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = am.assign(ctree, reads, genome, sel)
    off, lst = want["asg_off"], want["asg_sel"]
    rows = []
    for j, k in enumerate(sel):
        mine = [q for q in range(len(recs)) if j in lst[int(off[q]):int(off[q + 1])]]
        if mine:
            rows.append(",".join([ids[k]] + [n for q in mine for n in merge.get(recs[q][0], [])]))
    assert len(rows) > 3
    assert (out / "haplotype_reads.csv").read_text().splitlines() == rows
    cov = ["%s,%f" % (ids[k], want["sel_covered"][j] / genome) for j, k in enumerate(sel)]
    assert (out / "haplotype_coverage.csv").read_text().splitlines() == cov
    assert any(0 < c < genome for c in want["sel_covered"])
    # the map's files are written as before
    assert (out / "haplotype_scores.tsv").exists() and (out / "read_placements.tsv").exists()
    # an unknown or a repeated identifier is an error
    for bad in (ids[sel[0]] + "\nno_such_haplotype\n", ids[sel[0]] + "\n" + ids[sel[1 % K]] + "\n" + ids[sel[0]] + "\n"):
        sel_file.write_text(bad)
        r = subprocess.run(base + ["--assign", str(sel_file)], capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stderr
