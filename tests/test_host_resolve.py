"""`wepp-epp --assign FILE --resolve RESIDUAL`: mutation_reads.csv and mutation_haplotypes.csv (the files of
arena::resolve_unaccounted_mutations, src/WEPP/arena.cpp:698-904) on the fixture of test_host_assign.py, line for
line against the model of wepp_epp_resolve (tests/resolve_model.py); rows in the order of RESIDUAL."""
import subprocess

import numpy as np
import pytest

import pb_fixture as pbf
import resolve_cases as rc
import resolve_model as rm
import wepp_amd as w
from test_host_wepp import CLI, _as_reads, _condense, _setup, _sites

pytestmark = pytest.mark.gpu

LETTER = "NACMGRSVTWYHKDBN"


def test_resolve_files(tmp_path, oracle):
    rng = np.random.default_rng(79)
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
    sel_file.write_text("".join(ids[k] + "\n" for k in sel))

    code = {"A": 1, "C": 2, "G": 4, "T": 8}
    ref = {p: code[reference[p - 1]] for p in range(1, genome + 1)}
    residual = [r for r in rc.draw_residual(rng, reads, ref, genome, 40) if r[2] not in (7, 15)]
    # a mutation that only meets reads with an N at its site: in mutation_haplotypes.csv, not in mutation_reads.csv
    pos, _, mut, _ = w.unpack_read_word(reads.read_word)
    only_masked = None
    for p in sorted(set(pos[mut == 15].tolist())):
        free = [a for a in (1, 2, 4, 8) if a != ref[p] and not ((pos == p) & (mut == a)).any()]
        if free and not any(r[0] == p for r in residual):
            only_masked = (p, ref[p], free[0])
            break
    assert only_masked is not None
    residual.insert(len(residual) // 2, only_masked)
    residual = list(dict.fromkeys(residual))                      # (a repeated line is an error)
    values = ["%.2f" % rng.random() + (",%d" % m if m % 3 else "") for m in range(len(residual))]
    keys = ["%d%s:%s" % (p, LETTER[a], v.replace(",", ":")) for (p, _, a), v in zip(residual, values)]
    res_file = tmp_path / "residual_mutations.txt"
    res_file.write_text("".join("%d%s,%s\n" % (p, LETTER[a], v) for (p, _, a), v in zip(residual, values)))

    out = tmp_path / "out"; out.mkdir()
    plain = tmp_path / "plain"; plain.mkdir()
    base = [CLI, "-i", pb, "-r", rpb, "-f", fa, "-m", bed]
    r = subprocess.run(base + ["-d", str(out), "--assign", str(sel_file), "--resolve", str(res_file)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = rm.resolve(ctree, reads, genome, sel, residual)
    off, rel = want["rel_off"], want["rel_read"]
    rows_reads, rows_haps = [], []
    for m, key in enumerate(keys):
        mine = [int(x) for x in rel[int(off[m]):int(off[m + 1])]]
        covered = [x for x in mine if not x >> 31]
        if covered:
            rows_reads.append(",".join([key] + [n for q in covered for n in merge.get(recs[q][0], [])]))
        if mine:
            rows_haps.append(",".join([key] + [ids[sel[k]] for k in want["best"][m]]))
    m0 = residual.index(only_masked)
    assert int(want["n_covered"][m0]) == 0 and int(want["n_masked"][m0]) > 0
    assert len(rows_reads) > 5 and len(rows_haps) > len(rows_reads)
    assert any("_a," in row or row.endswith("_b") for row in rows_reads)
    assert (out / "mutation_reads.csv").read_text().splitlines() == rows_reads
    assert (out / "mutation_haplotypes.csv").read_text().splitlines() == rows_haps
    got_keys = [row.split(",")[0] for row in rows_haps]
    assert keys[m0] in got_keys and keys[m0] not in [row.split(",")[0] for row in rows_reads]

    # the files of --assign are what they are without --resolve
    r = subprocess.run(base + ["-d", str(plain), "--assign", str(sel_file)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("haplotype_reads.csv", "haplotype_coverage.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes(), name
    assert not (plain / "mutation_reads.csv").exists()

    # error exits
    r = subprocess.run(base + ["-d", str(out), "--resolve", str(res_file)], capture_output=True, text=True)
    assert r.returncode == 1 and "--resolve needs --assign" in r.stderr
    line = "%d%s,%s\n" % (residual[0][0], LETTER[residual[0][2]], values[0])
    for bad, what in ((line + "12A,0.5\n" + line, "more than once"), (line + "12A\n", "no comma"),
                      (line + "%dA,0.5\n" % (genome + 1), "outside the reference"), (line + "12N,0.5\n", "codec"),
                      (line + "12V,0.5\n", "codec"), (line + "A12,0.5\n", "<position><letter>")):
        res_file.write_text(bad)
        r = subprocess.run(base + ["-d", str(out), "--assign", str(sel_file), "--resolve", str(res_file)], capture_output=True, text=True)
        assert r.returncode == 1 and what in r.stderr, (bad, r.stderr)
