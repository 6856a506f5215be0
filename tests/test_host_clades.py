"""Clade annotations in the C++ host mirror: the loader's node_metadata.clade_annotations, Tree::get_clade_assignment,
the numbering and tables behind wepp_mat_set_clades (a program of its own, also under AddressSanitizer + UBSan),
the lineage names of `wepp-epp --clade-idx`; and on the GPU `wepp-usher` writing clades.txt (with and without -D) and
`wepp-epp --assign FILE --clade-idx N` writing the two proportion files -- against tests/clades_model.py."""
import os
import subprocess

import numpy as np
import pytest

import clades_cases as cc
import clades_model as cm
import fuzz_trees as ft
import pb_fixture as pbf
import wepp_amd as w
from test_host_cpp import CLI as USHER, _as_vcf_reader_sees, _expected_dump, _names, _tree_lists
from test_host_wepp import CLI as EPP, _as_reads, _condense, _setup, _sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "clades_host_main.cpp"), os.path.join(ROOT, "wepp_amd", "host", "mat.cpp")]


def write_annotated_pb(path, parent, names, muts, columns):
    """tests/pb_fixture.write_pb with columns[c][node] as the nodes' clade_annotations."""
    d = pbf.Data()
    d.newick, dfs = pbf.newick_and_dfs(parent, names)
    for i in dfs:
        lst = d.node_mutations.add()
        for (p, r, pa, mu) in muts[i]:
            m = lst.mutation.add()
            m.position = int(p)
            if p >= 0:
                m.ref_nuc = int(r).bit_length() - 1
                m.par_nuc = int(pa).bit_length() - 1
                m.mut_nuc.extend(b for b in range(4) if mu & (1 << b))
        d.metadata.add().clade_annotations.extend(col[i] for col in columns)
    open(path, "wb").write(d.SerializeToString())
    return dfs


def random_columns(rng, n, n_columns, p=0.35):
    return [[cc.POOL[int(rng.integers(0, len(cc.POOL)))] + (" x" if rng.random() < 0.1 else "") if rng.random() < p else ""
             for _ in range(n)] for _ in range(n_columns)]


def test_loader_reads_annotations(tmp_path):
    rng = np.random.default_rng(31)
    vcf = str(tmp_path / "s.vcf")
    pbf.write_vcf(vcf, ["s0"], [[(3, 1, 2, 0)]])
    for it, n_columns in enumerate([1, 3, 8, 2]):
        tree, _ref = ft.random_tree(rng, n_nodes=int(rng.integers(2, 70)))
        parent, muts = _tree_lists(tree)
        names = _names(parent)
        columns = random_columns(rng, len(parent), n_columns)
        pb = str(tmp_path / f"t{it}.pb")
        dfs = write_annotated_pb(pb, parent, names, muts, columns)
        newname = _expected_dump(parent, names, muts, dfs)
        out = subprocess.run([USHER, "-i", pb, "-v", vcf, "--dump"], check=True, capture_output=True, text=True).stdout.splitlines()
        assert f"annotations {n_columns}" in out
        got = {l.split("\t")[0][len("clade "):]: l.split("\t")[1:] for l in out if l.startswith("clade ")}
        assert len(got) == len(parent)
        for i in range(len(parent)):
            assert got[newname[i]] == [col[i] for col in columns], (it, i)
    # a .pb without metadata: no columns, as before
    pb = str(tmp_path / "plain.pb")
    pbf.write_pb(pb, [-1, 0, 0], ["r", "A", "B"], [[], [(10, 1, 1, 2)], []], metadata=False)
    out = subprocess.run([USHER, "-i", pb, "-v", vcf, "--dump"], check=True, capture_output=True, text=True).stdout
    assert "annotations" not in out and "clade " not in out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp(request.param) / "clades_host_main")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else ["-O2"]
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, *SRCS, "-o", out, "-lz"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return out


def test_clade_assignment_numbering_and_tables(exe, tmp_path):
    rng = np.random.default_rng(32)
    for it, n_columns in enumerate([1, 2, 8, 3]):
        tree, _ref = ft.random_tree(rng, n_nodes=int(rng.integers(1, 90)))
        parent, muts = _tree_lists(tree)
        columns = random_columns(rng, len(parent), n_columns, p=[0.0, 0.3, 0.6, 1.0][it])
        if it == 1:
            columns[0][0] = "UNDEFINED"                  # the reserved name as an annotation of its own
        pb = str(tmp_path / f"t{it}.pb")
        write_annotated_pb(pb, parent, _names(parent), muts, columns)
        r = subprocess.run([exe, pb], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert r.returncode == 0, r.stderr[-3000:]
        bfs, _kids = cm.bfs_order(parent)
        lines = r.stdout.splitlines()
        assert lines[0] == f"columns {n_columns}"
        _cid, und, want_names = w.number_clade_names(columns)
        names = [dict() for _ in range(n_columns)]
        for l in lines:
            if l.startswith("name "):
                head, nm = l.split("\t")
                names[int(head.split()[1])][int(head.split()[2])] = nm
        for c in range(n_columns):
            assert [names[c][i + 1] for i in range(len(names[c]))] == want_names[c]
        n_assign = n_table = 0
        for l in lines:
            if l.startswith("assign "):
                head, inc, exc = l.split("\t")
                c, i = int(head.split()[1]), int(head.split()[2])
                assert inc == cm.clade_assignment(parent, columns[c], bfs[i], True), (it, l)
                assert exc == cm.clade_assignment(parent, columns[c], bfs[i], False), (it, l)
                n_assign += 1
            elif l.startswith("table "):
                _t, c, i, inc, exc = l.split()
                c, i = int(c), int(i)
                assert names[c][int(inc)] == cm.clade_assignment(parent, columns[c], bfs[i], True), (it, l)
                assert names[c][int(exc)] == cm.clade_assignment(parent, columns[c], bfs[i], False), (it, l)
                if parent[bfs[i]] < 0:
                    assert int(exc) == int(und[c])
                n_table += 1
        assert n_assign == n_table == n_columns * len(parent)


def _lineage(parent, column, sources):
    """arena.cpp:462-483"""
    name = ""
    cur = sources[0]
    while cur >= 0:
        if column[cur] != "":
            name = column[cur]
            break
        cur = parent[cur]
    for s in sources[1:]:
        if column[s] != "":
            name += "/" + column[s]
    return name


def _epp_case(tmp_path, rng, n_nodes, n_reads, n_columns, p):
    mask = (15, 64)
    genome = 200
    tree, parent, muts, newname, reference, recs, pb, rpb, fa, bed = _setup(tmp_path, rng, n_nodes, n_reads, genome=genome, mask=mask)
    columns = random_columns(rng, len(parent), n_columns, p=p)
    write_annotated_pb(pb, parent, _names(parent), muts, columns)
    ents, start, end, degree = _as_reads(recs, reference, mask)
    cpar, cmuts, csrc, corig = _condense(parent, [[(m[0], m[1], m[3]) for m in ml] for ml in muts], _sites(ents, start, end, mask))
    return dict(parent=parent, columns=columns, newname=newname, csrc=csrc, corig=corig, cpar=cpar, cmuts=cmuts,
                base=[EPP, "-i", pb, "-r", rpb, "-f", fa, "-m", bed])


def test_lineage_names_of_condensed_nodes(tmp_path):
    rng = np.random.default_rng(33)
    k = _epp_case(tmp_path, rng, 250, 60, 2, 0.5)
    out = subprocess.run(k["base"] + ["--dump", "--clade-idx", "1"], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(l[len("lineage "):].split("\t") for l in out if l.startswith("lineage "))
    assert len(got) == len(k["csrc"])
    several = 0
    for h, sources in enumerate(k["csrc"]):
        want = _lineage(k["parent"], k["columns"][1], sources)
        assert got[k["newname"][k["corig"][h]]] == want, (h, sources)
        several += sum(1 for s in sources if k["columns"][1][s] != "") >= 2 and "/" in want
    assert several > 3
    # without the flag --dump prints what it printed before
    plain = subprocess.run(k["base"] + ["--dump"], check=True, capture_output=True, text=True).stdout
    assert "lineage " not in plain


def test_clade_idx_argument_errors(tmp_path):
    rng = np.random.default_rng(34)
    k = _epp_case(tmp_path, rng, 40, 20, 1, 0.5)
    r = subprocess.run(k["base"] + ["--clade-idx", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "--clade-idx needs --assign" in r.stderr
    for bad in ("x", "-1", "1.5", ""):
        r = subprocess.run(k["base"] + ["--assign", "whatever", "--clade-idx", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "--clade-idx needs a column number" in r.stderr, bad
    r = subprocess.run(k["base"] + ["--clade-idx"], capture_output=True, text=True)
    assert r.returncode == 1 and "needs a value" in r.stderr
    # a line of FILE without an abundance, or with one that is no number (checked before the device is touched)
    ident = k["newname"][k["corig"][0]]
    sel = tmp_path / "sel.txt"
    for text in (ident + "\n", ident + "\tabc\n", ident + ",\n"):
        sel.write_text(text)
        r = subprocess.run(k["base"] + ["-d", str(tmp_path), "--assign", str(sel), "--clade-idx", "0"], capture_output=True, text=True)
        assert r.returncode == 1 and "no abundance" in r.stderr, text


@pytest.mark.gpu
def test_wepp_usher_clades_txt(tmp_path, oracle):
    rng = np.random.default_rng(35)
    tree, ref = ft.random_tree(rng, n_nodes=220, genome=60, max_muts=2, p_root_masked=0.0)
    parent, muts = _tree_lists(tree)
    columns = random_columns(rng, len(parent), 3, p=0.4)
    samples = [ft.random_sample(rng, ref, genome=60, max_k=3) for _ in range(45)]
    snames = [f"s{i}" for i in range(45)]
    pb, vcf = str(tmp_path / "t.pb"), str(tmp_path / "s.vcf")
    write_annotated_pb(pb, parent, _names(parent), muts, columns)
    pbf.write_vcf(vcf, snames, samples)
    seen = [[_as_vcf_reader_sees(e) for e in s] for s in samples]
    ot = oracle.OracleTree(tree)
    best = cc.oracle_best(ot, seen)
    ot.close()
    per_sample = cc.expected(tree, columns, seen, best)[4]
    max_unc = sorted(b[1] for b in best)[len(best) * 2 // 3]
    placed = [q for q in range(45) if best[q][1] <= max_unc]
    assert 0 < len(placed) < 45 and any(best[q][1] > 1 for q in placed)
    assert any(len(set(names)) > 1 for q in placed for (_b, names) in per_sample[q])

    def run(name, *extra):
        out = tmp_path / name
        r = subprocess.run([USHER, "-i", pb, "-v", vcf, "-n", "-d", str(out), "-e", str(max_unc)] + list(extra), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert f"Writing clade annotations to file {out}/clades.txt \n" in r.stderr
        return out
    plain, detailed, two = run("plain"), run("detailed", "-D"), run("two", "--detailed-clades", "--devices", "0,0")
    assert (plain / "clades.txt").read_text() == "".join(cm.format_clades_row(snames[q], per_sample[q], False) for q in placed)
    want = "".join(cm.format_clades_row(snames[q], per_sample[q], True) for q in placed)
    assert (detailed / "clades.txt").read_text() == want
    assert (two / "clades.txt").read_text() == want
    assert (plain / "placement_stats.tsv").read_text() == (detailed / "placement_stats.tsv").read_text()
    # a tree without annotation columns, or with nothing but empty ones, writes no clades.txt
    for name, metadata in (("none", False), ("empty", True)):
        pbf.write_pb(pb, parent, _names(parent), muts, metadata=metadata)
        out = tmp_path / name
        r = subprocess.run([USHER, "-i", pb, "-v", vcf, "-n", "-D", "-d", str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and not (out / "clades.txt").exists() and "clade annotations" not in r.stderr
        assert (out / "placement_stats.tsv").exists()


@pytest.mark.gpu
def test_wepp_epp_proportion_files(tmp_path, oracle):
    rng = np.random.default_rng(36)
    k = _epp_case(tmp_path, rng, 250, 300, 2, 0.25)
    ctree = w.Tree.from_lists(k["cpar"], k["cmuts"])
    ot = oracle.OracleTree(ctree)
    order = [int(i) for i in ot.dfs_ids()]                       # condensed node with arena index a
    ot.close()
    K = min(24, len(order))
    sel = [order[int(a)] for a in rng.permutation(len(order))[:K]]
    abundance = [[0.25, 0.125, 0.5, 0.0625][j % 4] for j in range(K)]
    ids = [k["newname"][k["corig"][h]] for h in sel]
    sel_file = tmp_path / "selected.txt"
    sel_file.write_text("".join("%s%s%r%s\n" % (i, "\t," [j % 2], a, ("", ",more")[j % 3 == 0]) for j, (i, a) in enumerate(zip(ids, abundance))))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run(k["base"] + ["-d", str(out), "--assign", str(sel_file), "--clade-idx", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lineage = [_lineage(k["parent"], k["columns"][1], k["csrc"][h]) for h in sel]
    assert (out / "haplotype_proportion.csv").read_text().splitlines() == ["%s,%s,%f" % (i, l, a) for i, l, a in zip(ids, lineage, abundance)]
    sums = {}
    for l, a in zip(lineage, abundance):
        sums[l] = sums.get(l, 0.0) + a
    rows = sorted(sums.items(), key=lambda x: (-x[1], x[0]))
    assert len(rows) > 3 and any(a[1] == b[1] for a, b in zip(rows, rows[1:]))       # a tie in the sums
    assert (out / "lineage_proportion.csv").read_text().splitlines() == ["%s,%f" % (l, s) for l, s in rows]
    assert (out / "haplotype_reads.csv").exists()
    # a column the MAT does not have: the reference's error line, empty lineages, no lineage rows
    r = subprocess.run(k["base"] + ["-d", str(out), "--assign", str(sel_file), "--clade-idx", "2"], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR: CLADE_IDX = 2 exceeds Max CLADE_IDX = 1 in the MAT!!!" in r.stderr
    assert (out / "haplotype_proportion.csv").read_text().splitlines() == ["%s,,%f" % (i, a) for i, a in zip(ids, abundance)]
    assert (out / "lineage_proportion.csv").read_text() == ""
    # without --clade-idx the trailing text is ignored as before and the files are not written
    out2 = tmp_path / "out2"
    out2.mkdir()
    r = subprocess.run(k["base"] + ["-d", str(out2), "--assign", str(sel_file)], capture_output=True, text=True)
    assert r.returncode == 0 and not (out2 / "haplotype_proportion.csv").exists()
    assert (out2 / "haplotype_reads.csv").read_text() == (out / "haplotype_reads.csv").read_text()
