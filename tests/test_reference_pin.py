"""The oracle, the one-walk checker and the clade model against the REFERENCE's own compiled code.

tests/golden/ref_*.json were recorded by oracle/_ref/ref_driver (tests/ref_bridge.py: the reference's
usher_mapper.cpp and tree routines behind oracle/ref_driver.cpp); the fixture tests below need nothing but those
files.  test_live_differential builds or finds that binary and compares >= 20 000 fresh (tree, sample) pairs; it
skips only where the reference's sources are absent.  Integer work: every comparison is exact."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import clades_model as cm
import fuzz_trees as ft
import oracle_bridge as ob
import ref_bridge as rb
import ref_cases as rc

SCALARS = ("score", "num_best", "best_j", "has_unique")


def fnv(words):
    h = 1469598103934665603
    for w in words:
        h = ((h ^ (int(w) & 0xFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return str(h)


@pytest.fixture(scope="module")
def placement_cases():
    return rc.load("ref_mapper2") + rc.load("ref_digest")


@pytest.fixture(scope="module")
def clade_cases():
    return rc.load("ref_clades_hub") + rc.load("ref_clades_fuzz")


def _same_scalars(got, want, ctx):
    for k in SCALARS:
        assert int(got[k]) == want[k], (ctx, k, int(got[k]), want[k])
    assert got["best_j_vec"].tolist() == want["best_j_vec"], (ctx, "best_j_vec")


def _check_sample(ot, inc, case, q, r, lists, fixture=True):
    """One fixture sample against mapper2_oracle.c (ot) and incremental_oracle.c (inc), field by field"""
    cols = rc.columns_of([tuple(e) for e in r["sample"]])
    ref_p, ref_place = r["asc"].get("p"), r["asc"]["place"]        # (the clade fixtures keep the two-pass run alone)
    ctx = (case["name"], q)
    for name, side in (("oracle", ot), ("incremental", inc)):
        _same_scalars(side.place_sample(*cols, want_best_vec=True), ref_place, ctx + (name, "place"))
        if ref_p is None:
            continue
        got = side.place_sample(*cols, per_node_scores=True, want_best_vec=True)
        _same_scalars(got, ref_p, ctx + (name, "-p"))
        if "node_scores" in ref_p:
            assert got["node_scores"].tolist() == ref_p["node_scores"], ctx + (name, "node_scores")
    assert ot.imputed_at_node(*cols, ref_place["best_j"]) == [tuple(e) for e in ref_place["imputed_best"]], ctx
    if ref_p is None:
        return
    assert str(ot.lists_digest(*cols)) == ref_p["lists"], ctx + ("lists digest",)
    if fixture:
        # the digest of the excess lists alone, as the GPU test computes it from the library's lists
        per_node = [ot.lists_at_node(*cols, j)[0] for j in range(len(case["bfs_ids"]))]
        assert rc.excess_digest([[e for e in lst if e[0] >= 0] for lst in per_node]) == ref_p["excess_listed"], ctx
        assert sum(1 for lst in per_node for e in lst if e[0] < 0) == ref_p["excess_masked"], ctx
    if lists:
        for j in range(len(case["bfs_ids"])):
            exc, imp = ot.lists_at_node(*cols, j)
            assert exc == ref_p["excess"][j], ctx + (j, "excess")
            assert imp == ref_p["imputed"][j], ctx + (j, "imputed")
            # the entry point the GPU tests use (pass-2 form of the call): the same list
            assert [list(e) for e in ot.excess_at_node(*cols, j)] == ref_p["excess"][j], ctx + (j, "excess_at_node")


def test_fixtures_hold_the_kinds(placement_cases):
    """What the recorded inputs cover, counted on the inputs and the reference's own output"""
    n = dict(pairs=0, masked_root_zeroed=0, masked_root_nonzero=0, masked_node=0, ambiguous_tree_allele=0, ties=0,
             has_unique_0=0, has_unique_1=0, empty_sample=0, all_n_sample=0, with_lists=0)
    for case in placement_cases:
        t = case["tree"]
        zeroed, nonzero = rc.root_masked_kinds(case)
        root = t["parent"].index(-1)
        for r in case["results"]:
            n["pairs"] += 1
            n["masked_root_zeroed"] += zeroed
            n["masked_root_nonzero"] += nonzero
            n["ties"] += r["asc"]["place"]["num_best"] > 1
            n["has_unique_%d" % r["asc"]["place"]["has_unique"]] += 1
            n["empty_sample"] += not r["sample"]
            n["all_n_sample"] += bool(r["sample"]) and all(e[3] for e in r["sample"])
            n["with_lists"] += case["lists"]
        n["masked_node"] += any(p < 0 for i in range(len(t["parent"])) if i != root
                                for p in t["mut_pos"][t["mut_off"][i]:t["mut_off"][i + 1]])
        n["ambiguous_tree_allele"] += any(m & (m - 1) for m in t["mut_mut"])
    assert all(v > 0 for v in n.values()), n
    assert n["pairs"] >= 70 and n["with_lists"] >= 35, n


def test_oracles_match_the_reference_fixtures(placement_cases, clade_cases):
    n_pairs = 0
    for case in placement_cases + [c for c in clade_cases if not c.get("clades_only")]:
        ot = ob.OracleTree(rc.tree_of(case))
        inc = ot.incremental()
        assert ot.bfs_ids().tolist() == case["bfs_ids"], case["name"]
        for q, r in enumerate(case["results"]):
            _check_sample(ot, inc, case, q, r, case["lists"])
            n_pairs += 1
        inc.close()
        ot.close()
    assert n_pairs >= 140


def test_masked_root_with_nucleotides_is_counted_and_listed_by_the_reference(placement_cases):
    """usher_mapper.cpp:267-270, :402, :426-445: a masked ROOT mutation enters the ancestral set of the root alone;
    with ref_nuc != mut_nuc it costs the root one and is appended to its excess list as [position < 0, ref, mut,
    ref].  The .pb loader zeroes the three nucleotides (mutation_annotated_tree.cpp:583-588), so this needs a tree
    built in memory.  The oracle follows the reference here (the test above); wepp_excess_mutations documents that
    it does not list this one entry (include/wepp_place.h), and test_gpu_parity holds it to exactly that."""
    seen = 0
    for case in placement_cases:
        if not case["lists"]:
            continue
        t = case["tree"]
        root = t["parent"].index(-1)
        jr = case["bfs_ids"].index(root)
        want = [[t["mut_pos"][k], t["mut_ref"][k], t["mut_mut"][k], t["mut_ref"][k]]
                for k in range(t["mut_off"][root], t["mut_off"][root + 1])
                if t["mut_pos"][k] < 0 and t["mut_ref"][k] != t["mut_mut"][k]]
        for r in case["results"]:
            for j, exc in enumerate(r["asc"]["p"]["excess"]):
                masked = [e for e in exc if e[0] < 0]
                assert masked == (want if j == jr else []), (case["name"], j)
                seen += len(masked)
    assert seen > 0


def test_clades_model_matches_the_reference_fixtures(clade_cases):
    n = dict(pairs=0, columns=0, undefined=0, multi_run=0, include_self=0, exclude_self=0)
    fuzz = {p: dict(trees=0, ties=0, off_root=0, leaf=0, has_unique=0, walks_up=0) for p in ("none", "root", "all", "random")}
    for case in clade_cases:
        tree = rc.tree_of(case)
        parent, muts = cm.tree_lists(tree)
        bfs, kids = cm.bfs_order(parent)
        assert bfs == case["bfs_ids"]
        columns = case["columns"]
        for q, r in enumerate(case["results"]):
            sample = [tuple(e) for e in r["sample"]]
            ref = r["asc"]["place"]
            out, pairs = cm.assign_sample(parent, kids, muts, bfs, columns, sample, ref["best_j_vec"], ref["best_j"])
            # has_unique of every optimal node, as mapper2_body left it in node_has_unique
            assert [int(u) for (_n, _i, u) in pairs] == ref["node_has_unique"], (case["name"], q)
            assert len(out) == len(ref["clades"]) == len(columns)
            for c, ((best, names), (rbest, rnames)) in enumerate(zip(out, ref["clades"])):
                assert best == rbest and names == rnames, (case["name"], q, c)
                n["columns"] += 1
                n["undefined"] += best == "UNDEFINED"
                n["multi_run"] += len(set(names)) > 1
            if case["name"].startswith("clades_fuzz"):
                k = fuzz[case["note"].split()[-1]]
                k["ties"] += ref["num_best"] > 1
                k["off_root"] += any(parent[nd] >= 0 for (nd, _i, _u) in pairs)
                k["leaf"] += any(not kids[nd] and parent[nd] >= 0 for (nd, _i, _u) in pairs)
                k["has_unique"] += any(u for (_n, _i, u) in pairs)
                # an optimal node whose own annotation is not the answer: the walk goes to an ancestor
                k["walks_up"] += any(parent[nd] >= 0 and (not i or columns[0][nd] == "") for (nd, i, _u) in pairs)
            n["pairs"] += 1
            n["include_self"] += sum(1 for (_n, i, _u) in pairs if i)
            n["exclude_self"] += sum(1 for (nd, i, _u) in pairs if not i and kids[nd])
        if case["name"].startswith("clades_fuzz"):
            fuzz[case["note"].split()[-1]]["trees"] += 1
    assert all(v > 0 for v in n.values()), n
    # every annotation pattern of the fuzz trees meets ties, optimal nodes below the root, leaves, nodes with
    # has_unique set and walks to an ancestor
    assert all(v > 0 for k in fuzz.values() for v in k.values()) and sum(k["trees"] for k in fuzz.values()) >= 36, fuzz


def test_ascending_and_descending_node_orders_agree(placement_cases, clade_cases):
    """The reference visits the nodes in whatever order tbb::parallel_for deals them.  Serially ascending and serially
    descending, every recorded field is the same: the scalars, the sorted best_j_vec, node_has_unique of the optimal
    nodes, every node's -p score, the digest of all imputed and excess lists, the chosen node's imputed list and the
    clades.  (best_j_vec's own ORDER follows the schedule; the fixtures record it sorted, as DESIGN.md section 6
    says.)"""
    n = 0
    for case in placement_cases + clade_cases:
        for q, r in enumerate(case["results"]):
            a, d = r["asc"], r["desc"]
            for mode in ("p", "place") if "p" in a else ("place",):
                for k in SCALARS + ("best_j_vec", "node_has_unique"):
                    assert a[mode][k] == d[mode][k], (case["name"], q, mode, k)
            if "p" in a:
                assert a["p"]["lists"] == d["p"]["lists"], (case["name"], q)
                assert a["p"]["excess_listed"] == d["p"]["excess_listed"], (case["name"], q)
                if "node_scores" in d["p"]:
                    assert a["p"]["node_scores"] == d["p"]["node_scores"], (case["name"], q)
                else:
                    assert fnv(a["p"]["node_scores"]) == d["p"]["node_scores_digest"], (case["name"], q)
            assert a["place"]["imputed_best"] == d["place"]["imputed_best"], (case["name"], q)
            assert a["place"]["clades"] == d["place"]["clades"], (case["name"], q)
            n += 1
    assert n >= 200


# ---- live: fresh pairs through the binary -------------------------------------------------------------------------

CONFIGS = [(genome, max_muts, root_muts) for genome in (40, 60, 300) for max_muts in (2, 5) for root_muts in (True, False)]
TREES_PER_CONFIG = 42
SAMPLES_PER_TREE = 40


def _draw_batch(seed):
    """One tree of every configuration with its samples: [(tree, samples)]"""
    rng = np.random.default_rng(seed)
    batch = []
    for (genome, max_muts, root_muts) in CONFIGS:
        tree, ref = ft.random_tree(rng, n_nodes=int(rng.integers(1, 301)), genome=genome, max_muts=max_muts,
                                   root_muts=root_muts)
        samples = [ft.random_sample(rng, ref, genome=genome) for _ in range(SAMPLES_PER_TREE)]
        batch.append((tree, samples))
    return batch


def _run_batch(batch):
    enc = []
    for tree, samples in batch:
        parent, muts = rb.tree_lists(tree)
        enc.append((parent, muts, [], samples))
    return rb.run(enc, "digest")


def test_live_differential():
    """>= 20 000 (tree, sample) pairs of fuzz_trees through the reference binary, against both oracles: trees of 1 ..
    300 nodes, genomes 40 / 60 / 300, max_muts 2 / 5, root mutations on / off, every sample kind.  Compared per pair:
    the two-pass result and the -p result (score, num_best, best_j, has_unique, sorted best_j_vec, every node's
    score), node_has_unique of the optimal nodes against clades_model.has_unique, the digest of every node's imputed
    and excess list, and the descending run against the ascending one."""
    if rb.build() is None:
        pytest.skip("the reference's sources are not at %s (WEPP_REFERENCE_DIR)" % rb.REF_DIR)
    batches = [_draw_batch(5000 + i) for i in range(TREES_PER_CONFIG)]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        outs = list(pool.map(_run_batch, batches))
    n = dict(pairs=0, masked_root_zeroed=0, masked_root_nonzero=0, ambiguous_on_optimal_path=0, ties=0, has_unique_0=0,
             has_unique_1=0, empty_sample=0, all_n_sample=0, nodes_max=0, optimal_nodes=0)
    for batch, out in zip(batches, outs):
        for (tree, samples), rec in zip(batch, out):
            parent, muts = cm.tree_lists(tree)
            bfs, _kids = cm.bfs_order(parent)
            assert bfs == rec["bfs"]
            root = parent.index(-1)
            zeroed = any(m[0] < 0 and not (m[1] or m[2] or m[3]) for m in muts[root])
            nonzero = any(m[0] < 0 and m[1] != m[3] for m in muts[root])       # ref != mut: costs the root one, is listed
            ambig_path = [False] * len(parent)          # an ambiguous allele on the path root .. node (parent < node)
            for i in range(len(parent)):
                own = any(m[0] >= 0 and (m[3] & (m[3] - 1)) for m in muts[i])
                ambig_path[i] = own or (parent[i] >= 0 and ambig_path[parent[i]])
            ot = ob.OracleTree(tree)
            inc = ot.incremental()
            case = dict(name="live", bfs_ids=bfs)
            for q, (s, r) in enumerate(zip(samples, rec["results"])):
                r = dict(r, sample=s)
                _check_sample(ot, inc, case, q, r, False, fixture=False)
                a, d = r["asc"], r["desc"]
                for mode in ("p", "place"):
                    for k in SCALARS + ("best_j_vec", "node_has_unique"):
                        assert a[mode][k] == d[mode][k], (q, mode, k)
                assert a["p"]["lists"] == d["p"]["lists"] and fnv(a["p"]["node_scores"]) == d["p"]["node_scores_digest"]
                assert a["place"]["imputed_best"] == d["place"]["imputed_best"]
                place = a["place"]
                hu = [int(cm.has_unique(muts[bfs[j]], parent[bfs[j]] < 0, s)) for j in place["best_j_vec"]]
                assert hu == place["node_has_unique"], (q, "node_has_unique")
                n["pairs"] += 1
                n["masked_root_zeroed"] += zeroed
                n["masked_root_nonzero"] += nonzero
                n["ambiguous_on_optimal_path"] += any(ambig_path[bfs[j]] for j in place["best_j_vec"])
                n["ties"] += place["num_best"] > 1
                n["has_unique_%d" % place["has_unique"]] += 1
                n["empty_sample"] += not s
                n["all_n_sample"] += bool(s) and all(e[3] for e in s)
                n["optimal_nodes"] += place["num_best"]
            n["nodes_max"] = max(n["nodes_max"], len(parent))
            inc.close()
            ot.close()
    print("live differential:", n)
    assert n["pairs"] >= 20000, n
    assert all(v > 0 for v in n.values()), n
    assert n["nodes_max"] >= 250, n
