"""`wepp-epp --assign FILE --uncertainty --haplotypes --truth TRUE`: haplotype_uncertainty.csv, haplotypes.tsv and the
lines of print_mutation_distance (arena::dump_haplotype_uncertainty, dump_haplotypes, print_mutation_distance,
src/WEPP/arena.cpp:494-528, 906-931, 251-301) byte for byte against the literal model (tests/geno_model.py), on a
tree whose reads cover a tenth of the genome: condensing merges one source, several, and more than 64 into a node."""
import subprocess

import numpy as np
import pytest

import geno_model as gm
import pb_fixture as pbf
from test_host_wepp import CH, CLI, _as_reads, _condense, _setup, _sites

pytestmark = pytest.mark.gpu


def test_uncertainty_haplotypes_truth(tmp_path):
    rng = np.random.default_rng(411)
    genome = 200
    tree, parent, muts, newname, reference, _, pb, rpb, fa, bed = _setup(tmp_path, rng, 700, 1, genome=genome)
    # reads over sites 11 .. 30 only: the reference with a few substitutions and N's
    recs = []
    for q in range(60):
        s = int(rng.integers(11, 25))
        e = min(30, s + int(rng.integers(3, 20)))
        content = [reference[p - 1] if rng.random() > 0.1 else "ACGTN"[int(rng.integers(0, 5))] for p in range(s, e + 1)]
        recs.append(("read_%d" % q, s, "".join(content), 1 + q % 3))
    pbf.write_reads_pb(rpb, recs, {})
    ents, start, end, degree = _as_reads(recs, reference)
    sites = _sites(ents, start, end)
    assert sites and max(sites) <= 30 and min(sites) >= 11
    cpar, cmuts, csrc, corig = _condense(parent, [[(m[0], m[1], m[3]) for m in ml] for ml in muts], sites)
    size = [len(s) for s in csrc]
    big = [k for k in range(len(csrc)) if size[k] > 64]
    some = [k for k in range(len(csrc)) if 2 <= size[k] <= 64]
    one = [k for k in range(len(csrc)) if size[k] == 1]
    assert big and len(some) >= 3 and len(one) >= 3, size
    sel = [some[0], big[0], one[0], some[1], one[1], some[2], one[2]] + some[3:12]
    ids = [newname[corig[k]] for k in sel]
    sel_file, truth_file = tmp_path / "selected.txt", tmp_path / "truth.txt"
    sel_file.write_text("".join(i + "\n" for i in ids))
    true_nodes = [int(x) for x in rng.permutation(tree.n_nodes)[:25]]
    truth_file.write_text("".join(newname[t] + "\n" for t in true_nodes))
    out = tmp_path / "out"
    out.mkdir()
    base = [CLI, "-i", pb, "-r", rpb, "-f", fa, "-d", str(out)]
    r = subprocess.run(base + ["--assign", str(sel_file), "--uncertainty", "--haplotypes", "--truth", str(truth_file)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = "".join(gm.uncertainty_row(tree, newname, csrc[k]) for k in sel)
    assert (out / "haplotype_uncertainty.csv").read_text() == want
    assert any(row.split(",")[0] not in ("0", "1") for row in want.splitlines())          # distances worth the name
    want = "".join(gm.haplotype_row(newname[corig[k]], "ref", reference, gm.get_mutations(tree, corig[k])) for k in sel)
    assert (out / "haplotypes.tsv").read_text() == want
    lines, avg = gm.truth_lines(tree, newname, true_nodes, [corig[k] for k in sel], sites)
    want = "--- ground truth %d haps; predicted %d haps\n" % (len(true_nodes), len(sel)) + "".join(lines) + "average mutation_distance: %0.3f\n" % avg
    assert r.stdout == want
    # each flag needs --assign; an unknown or repeated true node is an error
    for flags in (["--uncertainty"], ["--haplotypes"], ["--truth", str(truth_file)]):
        r = subprocess.run(base + flags, capture_output=True, text=True)
        assert r.returncode == 1 and flags[0] + " needs --assign" in r.stderr
    for bad in (newname[true_nodes[0]] + "\nno_such_node\n", newname[true_nodes[0]] + "\n" + newname[true_nodes[0]] + "\n"):
        truth_file.write_text(bad)
        r = subprocess.run(base + ["--assign", str(sel_file), "--truth", str(truth_file)], capture_output=True, text=True)
        assert r.returncode == 1 and "ERROR" in r.stderr
