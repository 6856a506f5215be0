"""`wepp-sam2pb --subsample-seed`: more mapped reads than --max-reads are subsampled through
wepp_sam_build_subsampled and the file is written from the kept reads.  The decoded message equals the model
(tests/subsample_model.py) in reads, names, degrees and reverse columns; --dump writes the full raw table and
subsample_trials.tsv; two runs write the same bytes; `wepp-epp -r` reads the file to the end; without the seed the same
command fails as it always did."""
import subprocess

import numpy as np
import pytest

import sam_model as sm
import subsample_model as sub
from test_host_sam2pb import CLI, GENOME, OPTS, decode
from test_host_wepp import CLI as EPP_CLI, _setup

pytestmark = pytest.mark.gpu

SEED, TRIALS = 20250, 30


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam2pb_sub")
    tree, parent, muts, newname, reference, recs, pb, rpb, fa, bed = _setup(d, np.random.default_rng(5), 150, 5, genome=GENOME)
    _, text = sm.gen_sam(11, G=GENOME, n_lines=400)
    aligned = sm.parse_sam(text, GENOME, 20)
    assert len(aligned) >= 400
    (d / "in.sam").write_text(text)
    return dict(dir=d, reference=reference, fa=fa, pb=pb, aligned=aligned)


def command(fixture, out, m, seed=True):
    d = fixture["dir"]
    cmd = [CLI, "-s", str(d / "in.sam"), "-f", fixture["fa"], "-o", str(out), "--max-reads", str(m)] + OPTS
    return cmd + (["--subsample-seed", str(SEED), "--subsample-trials", str(TRIALS)] if seed else [])


@pytest.mark.parametrize("which", ["n-1", "n/2"])
def test_written_message_equals_the_model(fixture, which):
    d, aligned = fixture["dir"], fixture["aligned"]
    n = len(aligned)
    m = n - 1 if which == "n-1" else n // 2
    model = sub.subsample(fixture["reference"], aligned, sm.stof("0.05"), 2, SEED, m, TRIALS)
    slack = sub.separated(model)
    assert slack is not None and slack > 0, "the winner is not separated: change SEED"
    assert 1 < len(model["start"]) < m and max(model["degree"]) > 1
    dump = d / f"dump_{m}"
    dump.mkdir()
    out = d / f"sub_{m}.pb"
    r = subprocess.run(command(fixture, out, m) + ["--dump", str(dump)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stderr.splitlines() if "subsampled" in ln]
    assert len(line) == 1 and f"subsampled {m} of {n} mapped reads: trial {model['best_trial']} of {TRIALS}, divergence " in line[0]
    assert abs(float(line[0].rsplit(" ", 1)[1]) - model["divergence"][model["best_trial"]]) <= model["bound"][model["best_trial"]]
    msg = decode(out)
    got = [(x.read, x.start_idx, x.content, x.degree) for x in msg.reads]
    assert got == list(zip(model["name"], model["start"], model["content"], model["degree"]))
    assert [(c.column_name, list(c.input_columns)) for c in msg.reverse_columns] == sorted(model["reverse_columns"].items())
    assert sum(len(c.input_columns) for c in msg.reverse_columns) == m
    # the dumped table is the FULL raw table
    rows = ["Position\tAllele\tFrequency\tDepth"]
    for site, f in enumerate(model["freq"]):
        for cnt, j in sorted(((f[j], j) for j in range(6) if f[j]), reverse=True):
            rows.append("%d\t%s\t%.10f\t%d" % (site + 1, sm.GENOME_STRING[j], cnt / sum(f), sum(f)))
    assert (dump / "frequency_table.tsv").read_text().splitlines() == rows
    tsv = [ln.split("\t") for ln in (dump / "subsample_trials.tsv").read_text().splitlines()]
    assert tsv[0] == ["trial", "divergence", "chosen"] and len(tsv) == TRIALS + 1
    for t, row in enumerate(tsv[1:]):
        assert int(row[0]) == t and int(row[2]) == (t == model["best_trial"])
        assert abs(float(row[1]) - model["divergence"][t]) <= model["bound"][t], (t, row[1], model["divergence"][t])
        assert row[1] == "%.17g" % float(row[1])
    # a second run writes the same bytes
    again = d / f"again_{m}.pb"
    r = subprocess.run(command(fixture, again, m), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(again, "rb").read() == open(out, "rb").read()


def test_wepp_epp_reads_the_file(fixture):
    d = fixture["dir"]
    m = len(fixture["aligned"]) // 2
    out = d / "for_epp.pb"
    r = subprocess.run(command(fixture, out, m), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n_merged = len(decode(out).reads)
    res = d / "epp_out"
    res.mkdir()
    r = subprocess.run([EPP_CLI, "-i", fixture["pb"], "-r", str(out), "-f", fixture["fa"], "-d", str(res)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert len((res / "read_placements.tsv").read_text().splitlines()) >= n_merged


def test_without_the_seed_it_fails_as_before(fixture):
    d = fixture["dir"]
    out = d / "never.pb"
    r = subprocess.run(command(fixture, out, len(fixture["aligned"]) - 1, seed=False), capture_output=True, text=True)
    assert r.returncode != 0 and "--max-reads" in r.stderr and "nothing was written" in r.stderr and not out.exists()


def test_seed_and_few_reads_is_the_plain_build(fixture):
    """with a seed but no more reads than --max-reads nothing is drawn: the same bytes as without the seed"""
    d, n = fixture["dir"], len(fixture["aligned"])
    a, b = d / "plain.pb", d / "seeded.pb"
    r = subprocess.run(command(fixture, a, n, seed=False), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(command(fixture, b, n), capture_output=True, text=True)
    assert r.returncode == 0 and "subsampled" not in r.stderr, r.stderr
    assert open(a, "rb").read() == open(b, "rb").read()
