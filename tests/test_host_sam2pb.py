"""`wepp-sam2pb`: SAM text (plain and .gz) -> reads .pb[.gz].  The written message, decoded with the protobuf runtime
(tests/pb_fixture.py), equals tests/sam_model.py in reads, names, degrees and reverse columns; --dump writes the raw
frequency table; `wepp-epp -r` runs to the end on the file; more mapped reads than --max-reads is an error that writes
nothing.  And the merged batch wepp_sam_build delivers gives wepp_epp_map the same outputs, byte for byte, as the batch
load_reads_from_proto builds from the written file."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import pb_fixture as pbf
import sam_model as sm
import wepp_amd as w
from test_host_wepp import CLI as EPP_CLI, _as_reads, _setup
from test_sam_gpu import encode

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wepp_amd", "wepp-sam2pb")
GENOME = 200
OPTS = ["--min-af", "0.05", "--min-depth", "2", "--min-phred", "20"]


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam2pb")
    tree, parent, muts, newname, reference, recs, pb, rpb, fa, bed = _setup(d, np.random.default_rng(5), 150, 5, genome=GENOME)
    _, text = sm.gen_sam(11, G=GENOME, n_lines=400)
    aligned = sm.parse_sam(text, GENOME, 20)
    model = sm.build(reference, aligned, sm.stof("0.05"), 2)
    assert len(aligned) >= 400 and 1 < len(model["start"]) < len(aligned) and max(model["degree"]) > 1
    assert any(a[2] != c[2] for a, c in zip(aligned, model["corrected"]))
    (d / "in.sam").write_text(text)
    (d / "in.sam.gz").write_bytes(gzip.compress(text.encode()))
    return dict(dir=d, tree=tree, reference=reference, fa=fa, pb=pb, aligned=aligned, model=model)


def decode(path):
    raw = open(path, "rb").read()
    msg = pbf.Sam()
    msg.ParseFromString(gzip.decompress(raw) if str(path).endswith(".gz") else raw)
    return msg


@pytest.mark.parametrize("inp,out", [("in.sam", "reads.pb"), ("in.sam.gz", "reads.pb.gz")])
def test_written_message_equals_the_model(fixture, inp, out):
    d, m = fixture["dir"], fixture["model"]
    dump = d / ("dump_" + inp)
    dump.mkdir()
    r = subprocess.run([CLI, "-s", str(d / inp), "-f", fixture["fa"], "-o", str(d / out), "--dump", str(dump)] + OPTS, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(d / out, "rb").read()
    assert (raw[:2] == b"\x1f\x8b") == out.endswith(".gz")
    msg = decode(d / out)
    got = [(x.read, x.start_idx, x.content, x.degree) for x in msg.reads]
    assert got == list(zip(m["name"], m["start"], m["content"], m["degree"]))
    assert [(c.column_name, list(c.input_columns)) for c in msg.reverse_columns] == sorted(m["reverse_columns"].items())
    # the raw table in the layout of dump_sub_table: alleles of a site by descending count, then descending column
    rows = ["Position\tAllele\tFrequency\tDepth"]
    for site, f in enumerate(m["freq"]):
        for cnt, j in sorted(((f[j], j) for j in range(6) if f[j]), reverse=True):
            rows.append("%d\t%s\t%.10f\t%d" % (site + 1, sm.GENOME_STRING[j], cnt / sum(f), sum(f)))
    assert (dump / "frequency_table.tsv").read_text().splitlines() == rows


def test_wepp_epp_reads_the_file(fixture):
    d = fixture["dir"]
    r = subprocess.run([CLI, "-s", str(d / "in.sam"), "-f", fixture["fa"], "-o", str(d / "for_epp.pb")] + OPTS, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = d / "epp_out"
    out.mkdir()
    r = subprocess.run([EPP_CLI, "-i", fixture["pb"], "-r", str(d / "for_epp.pb"), "-f", fixture["fa"], "-d", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert len((out / "read_placements.tsv").read_text().splitlines()) >= len(fixture["model"]["start"])


def test_more_reads_than_max_reads(fixture):
    d = fixture["dir"]
    out = d / "never.pb"
    r = subprocess.run([CLI, "-s", str(d / "in.sam"), "-f", fixture["fa"], "-o", str(out), "--max-reads", str(len(fixture["aligned"]) - 1)] + OPTS,
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--max-reads" in r.stderr and "nothing was written" in r.stderr and not out.exists()
    r = subprocess.run([CLI, "-s", str(d / "in.sam"), "-f", fixture["fa"], "-o", str(out), "--max-reads", str(len(fixture["aligned"]))] + OPTS,
                       capture_output=True, text=True)
    assert r.returncode == 0 and out.exists(), r.stderr


def test_merged_batch_maps_like_the_loaded_file(fixture):
    d, ref = fixture["dir"], fixture["reference"]
    r = subprocess.run([CLI, "-s", str(d / "in.sam"), "-f", fixture["fa"], "-o", str(d / "for_map.pb")] + OPTS, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    recs = [(x.read, x.start_idx, x.content, x.degree) for x in decode(d / "for_map.pb").reads]
    loaded = w.EppReads.from_lists(*_as_reads(recs, ref))
    built = w.sam_build(ref, *encode(fixture["aligned"]), min_af=sm.stof("0.05"), min_depth=2)["reads"]
    assert loaded.n_reads == built.n_reads > 1 and loaded.read_word.size > 0
    mat = w.Mat(fixture["tree"])
    a, b = mat.epp_map(built, GENOME), mat.epp_map(loaded, GENOME)
    mat.close()
    for k in ("max_parsimony", "multiplicity", "score", "counts", "divergence", "epp_off", "epp_nodes"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
