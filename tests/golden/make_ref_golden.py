"""Generates tests/golden/ref_*.json: inputs and what the REFERENCE's own code recorded for them.

The numbers come from oracle/_ref/ref_driver (tests/ref_bridge.py): the reference's usher_mapper.cpp and tree routines,
compiled from where the reference's sources lie, behind oracle/ref_driver.cpp.  Nothing here is produced by
oracle/mapper2_oracle.c, tests/clades_model.py or the library; tests/test_reference_pin.py and the GPU tests hold
those to these files.  Needs the reference's sources (WEPP_REFERENCE_DIR); the committed files do not.

  ref_mapper2_*.json      the hand cases of make_golden.py and three small trees of fuzz_trees.random_tree with its
                          default switches (a masked root mutation of either kind, a masked node, ambiguous alleles), 4
                          samples each; -p mode and two-pass mode, nodes ascending and descending, with the imputed and
                          excess list of every (sample, node) pair of the ascending -p run
  ref_digest_*.json       eight more default fuzz trees and one of 150 .. 200 nodes (genome 300); the same with
                          digests in place of the lists
  ref_clades_hub_*.json   clades_cases.hub_tree at small segment sizes: every annotation pattern at 2 columns, the mixed
                          one at 1 and 8
  ref_clades_fuzz_*.json  small annotated fuzz trees in the patterns of test_clades_gpu.test_fuzz_trees

Run from the repo root:  python tests/golden/make_ref_golden.py
"""
import glob
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import clades_cases as cc        # noqa: E402
import fuzz_trees as ft          # noqa: E402
import make_golden as mg         # noqa: E402
import ref_bridge as rb          # noqa: E402

LIMIT = 120_000                  # bytes per file, below the 127 KB of mapper2_cases.json
HUB_SIZES = [1, 2, 64, 65]           # both sides of 1 key | a wave | a workgroup (clades.hpp)
GENERATOR = "tests/golden/make_ref_golden.py (oracle/_ref/ref_driver: the reference's usher_mapper.cpp and tree routines)"


def sample_lists(samples):
    return [[[int(x) for x in (e + (0,))[:4]] for e in s] for s in samples]


def run_cases(inputs, mode):
    """inputs: [(name, note, tree, columns, samples)] -> fixture cases with the driver's output"""
    enc = []
    for (_name, _note, tree, columns, samples) in inputs:
        parent, muts = rb.tree_lists(tree)
        enc.append((parent, muts, columns, samples))
    outs = rb.run(enc, mode)
    cases = []
    for (name, note, tree, columns, samples), out in zip(inputs, outs):
        results = [dict(sample=s, asc=r["asc"], desc=r["desc"]) for s, r in zip(sample_lists(samples), out["results"])]
        cases.append(dict(name=name, note=note, tree=mg.tree_to_json(tree), columns=columns, bfs_ids=out["bfs"],
                          lists=(mode == "full"), results=results))
    return cases


def run_lengths(case):
    """The sorted clade lists as [name, count] runs (ref_cases.load() expands them again): the hub's lists are long"""
    for r in case["results"]:
        for order in ("asc", "desc"):
            place = r[order]["place"]
            rle = []
            for (best, names) in place.pop("clades"):
                runs = []
                for nm in names:
                    if runs and runs[-1][0] == nm:
                        runs[-1][1] += 1
                    else:
                        runs.append([nm, 1])
                rle.append([best, runs])
            place["clades_rle"] = rle
    return case


def clades_only(case, base_name):
    """A further annotation of the tree and samples of case `base_name`: the columns and the clades alone"""
    res = [dict(asc=dict(place=dict(clades_rle=r["asc"]["place"]["clades_rle"])),
                desc=dict(place=dict(clades_rle=r["desc"]["place"]["clades_rle"]))) for r in case["results"]]
    return dict(name=case["name"], note=case["note"], same_tree_as=base_name, columns=case["columns"], results=res)


def write_split(prefix, cases):
    """cases into prefix_NN.json files of at most LIMIT bytes; a clades-only case stays in the file of its tree"""
    files, cur = [], []
    for case in cases:
        trial = cur + [case]
        if cur and "same_tree_as" not in case and len(json.dumps(dict(generator=GENERATOR, cases=trial), separators=(",", ":"))) > LIMIT:
            files.append(cur)
            cur = [case]
        else:
            cur = trial
    if cur:
        files.append(cur)
    for i, chunk in enumerate(files):
        path = os.path.join(HERE, "%s_%02d.json" % (prefix, i))
        with open(path, "w") as fh:
            json.dump(dict(generator=GENERATOR, cases=chunk), fh, separators=(",", ":"))
        size = os.path.getsize(path)
        print("wrote", os.path.basename(path), size, "bytes,", len(chunk), "cases")
        assert size <= 127_000, path


def hub_samples(info, rng):
    samples = []
    for g in info["groups"]:
        samples += [g["sample"], []]
    samples += [info["probe_shared"], info["probe_unique"], [(5, cc.A, cc.C, 0), (10, cc.A, cc.C, 0)], [(11, cc.A, cc.G, 0)]]
    order = rng.permutation(len(samples))
    return [samples[int(i)] for i in order]


def main():
    if rb.build() is None:
        sys.exit("the reference's sources are not at %s" % rb.REF_DIR)
    for old in glob.glob(os.path.join(HERE, "ref_*.json")):
        os.remove(old)
    rng = np.random.default_rng(20261020)

    # default switches throughout; WHICH of the drawn trees get their lists written out is decided on the inputs alone:
    # the first small ones that hold a masked root mutation with nucleotides (ref != mut), a zeroed one, and a masked node with an
    # ambiguous allele.  The eight trees drawn after them keep digests of their lists.
    def root_masked(tree, nonzero):
        _p, muts = rb.tree_lists(tree)
        return any(m[0] < 0 and (m[1] != m[3] if nonzero else not (m[1] or m[2] or m[3])) for m in muts[0])

    def masked_node_and_ambiguous(tree):
        _p, muts = rb.tree_lists(tree)
        return any(m[0] < 0 for ml in muts[1:] for m in ml) and any(m[0] >= 0 and m[3] & (m[3] - 1) for ml in muts for m in ml)
    wanted = [lambda t: root_masked(t, True), lambda t: root_masked(t, False), masked_node_and_ambiguous]
    inputs = [("hand_" + name, note, tree, [], samples) for (name, tree, samples, note) in mg.hand_case_inputs()]
    while wanted:
        tree, ref = ft.random_tree(rng)
        samples = [ft.random_sample(rng, ref) for _ in range(4)]
        if 6 <= tree.n_nodes <= 14 and wanted[0](tree):
            wanted.pop(0)
            inputs.append(("fuzz_lists_%d" % len(wanted), "", tree, [], samples))
    write_split("ref_mapper2", run_cases(inputs, "full"))
    inputs = []
    for i in range(8):
        tree, ref = ft.random_tree(rng)
        inputs.append(("fuzz_%d" % i, "", tree, [], [ft.random_sample(rng, ref) for _ in range(4)]))
    for i, (genome, max_muts, root_muts) in enumerate([(300, 5, True)]):
        tree, ref = ft.random_tree(rng, n_nodes=int(rng.integers(150, 201)), genome=genome, max_muts=max_muts,
                                   root_muts=root_muts, p_root_masked=1.0 if root_muts else 0.0)
        inputs.append(("large_%d" % i, "genome %d max_muts %d root_muts %s" % (genome, max_muts, root_muts), tree, [],
                       [ft.random_sample(rng, ref, genome=genome) for _ in range(4)]))
    write_split("ref_digest", run_cases(inputs, "digest"))

    tree, info = cc.hub_tree(HUB_SIZES)
    parent = [int(p) for p in tree.parent]
    samples = hub_samples(info, rng)
    inputs = []
    for n_columns, patterns in ((2, ("none", "root", "all", "mixed")), (1, ("mixed",)), (8, ("mixed",))):
        for pattern in patterns:
            columns = cc.annotate(info["kind"], parent, n_columns, pattern, np.random.default_rng(n_columns))
            inputs.append(("hub_%d_%s" % (n_columns, pattern), "hub_tree(%r)" % HUB_SIZES, tree, columns, samples))
    cases = [run_lengths(c) for c in run_cases(inputs, "digest")]
    for r in cases[0]["results"]:         # the clade fixtures keep the two-pass runs alone
        r["asc"].pop("p"), r["desc"].pop("p")
    write_split("ref_clades_hub", [cases[0]] + [clades_only(c, cases[0]["name"]) for c in cases[1:]])

    inputs = []
    for it in range(36):                  # as many as test_clades_gpu.test_fuzz_trees draws, in its patterns
        tree, ref = ft.random_tree(rng, n_nodes=int(rng.integers(8, 31)), genome=40, max_muts=2)
        parent = [int(p) for p in tree.parent]
        n = tree.n_nodes
        n_columns = [1, 2, 8][it % 3]
        pattern = ["none", "root", "all", "random"][(it // 3) % 4]
        if pattern == "random":
            columns = [[cc.POOL[int(rng.integers(0, len(cc.POOL)))] if rng.random() < 0.4 else "" for _ in range(n)]
                       for _ in range(n_columns)]
        else:
            columns = cc.annotate(["root" if p < 0 else "node" for p in parent], parent, n_columns, pattern, rng)
        inputs.append(("clades_fuzz_%d" % it, "%d columns, %s" % (n_columns, pattern), tree, columns,
                       [ft.random_sample(rng, ref, genome=40, max_k=4) for _ in range(5)]))
    cases = [run_lengths(c) for c in run_cases(inputs, "digest")]
    for c in cases:
        for r in c["results"]:
            r["asc"].pop("p"), r["desc"].pop("p")
    for pattern in ("none", "root", "all", "random"):     # (tests/test_reference_pin.py asserts the same on the files)
        runs = [r["asc"]["place"] for c in cases if c["note"].endswith(pattern) for r in c["results"]]
        assert any(p["num_best"] > 1 for p in runs) and any(j != 0 for p in runs for j in p["best_j_vec"]), pattern
    write_split("ref_clades_fuzz", cases)


if __name__ == "__main__":
    main()
