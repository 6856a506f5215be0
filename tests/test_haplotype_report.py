"""The host routines behind --uncertainty / --haplotypes / --truth (wepp_amd/host/haplotype_report.cpp) as a
stand-alone program (tests/cxx/haplotype_report_main.cpp), plain and under AddressSanitizer + UBSan, against the
literal model (tests/geno_model.py): get_mutations, the packed words, the MD string and the row formats, the FASTA
header token, the keep mask."""
import os
import subprocess

import numpy as np
import pytest

import fuzz_trees as ft
import geno_model as gm
import pb_fixture as pbf
from test_host_cpp import _names, _tree_lists, _expected_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "haplotype_report_main.cpp"), os.path.join(ROOT, "wepp_amd", "host", "haplotype_report.cpp"),
        os.path.join(ROOT, "wepp_amd", "host", "mat.cpp")]
CH = {1: "A", 2: "C", 4: "G", 8: "T"}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp(request.param) / "haplotype_report_main")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + SRCS + ["-o", out, "-lz"])
    return out


def case(tmp_path, seed, n_nodes, genome, header):
    rng = np.random.default_rng(seed)
    tree, ref = ft.random_tree(rng, n_nodes=n_nodes, genome=genome, p_root_masked=0.0, p_ambig=0.0)   # (a .pb holds one-hot parent alleles only)
    parent, muts = _tree_lists(tree)
    names = _names(parent)
    pb, fa = str(tmp_path / ("t%d.pb" % seed)), str(tmp_path / ("r%d.fa" % seed))
    dfs = pbf.write_pb(pb, parent, names, muts)
    newname = _expected_dump(parent, names, muts, dfs)
    reference = "".join(CH[ref[p]] for p in range(1, genome + 1))
    open(fa, "w").write(header + "\n" + "\n".join(reference[i:i + 37].lower() for i in range(0, genome, 37)) + "\n")
    return tree, dfs, newname, reference, pb, fa


@pytest.mark.parametrize("seed,n_nodes,genome,header,ref_name", [(1, 80, 30, ">NC_045512v2 Severe acute", "NC_045512v2"),
                                                                 (2, 1, 8, ">x", "x"), (3, 200, 12, ">  spaced\tname", "spaced")])
def test_against_model(program, tmp_path, seed, n_nodes, genome, header, ref_name):
    tree, dfs, ids, reference, pb, fa = case(tmp_path, seed, n_nodes, genome, header)
    r = subprocess.run([program, pb, fa], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    geno = [gm.get_mutations(tree, n) for n in dfs]
    want = ["name " + ref_name]
    want += ["geno " + " ".join([ids[n]] + ["%d:%d:%d" % e for e in g]) for n, g in zip(dfs, geno)]
    off, words = gm.pack(geno)
    for k, n in enumerate(dfs):
        o = (k + 7) % len(dfs)
        want.append(" ".join(["words " + ids[n]] + [str(int(x)) for x in words[int(off[k]):int(off[k + 1])]]))
        want.append("row " + gm.haplotype_row(ids[n], ref_name, reference, geno[k])[:-1])
        want.append("dist %s %s %d" % (ids[n], ids[dfs[o]], gm.distance(geno[k], geno[o])))
        want.append("dist %s %s %d" % (ids[dfs[o]], ids[n], gm.distance(geno[o], geno[k])))
        src = [n] + ([int(tree.parent[n]), dfs[0]] if tree.parent[n] >= 0 else [])
        want.append("unc " + ",".join([str(k)] + [ids[s] for s in src]))
        want.append("truth * dist: %02d true_node: %s pred_node: %s " % (k % 120, ids[n], ids[dfs[o]]))
    sites = set(p for p, _, _ in geno[-1])
    kp = max(sites) + 1 if sites else 0
    want.append(" ".join(["keep %d" % kp] + ["%x" % int(b) for b in gm.keep_bits(sites, kp)]))
    assert r.stdout.split("\n")[:-1] == want
    assert n_nodes == 1 or any(len(g) > 2 for g in geno)


def test_bad_fasta_is_an_error(program, tmp_path):
    tree, dfs, ids, reference, pb, fa = case(tmp_path, 5, 3, 8, "no header mark")
    r = subprocess.run([program, pb, fa], capture_output=True, text=True)
    assert r.returncode == 1 and "Fasta format NOT correct" in r.stderr
