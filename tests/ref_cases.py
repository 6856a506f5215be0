"""The reference-made fixtures tests/golden/ref_*.json (written by tests/golden/make_ref_golden.py with the
reference's own compiled scorer) as the tests read them."""
import glob
import json
import os

from wepp_amd import Tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(prefix):
    """The cases of golden/<prefix>_*.json in file order.  A case that only annotates another case's tree anew
    (`same_tree_as`) gets that case's tree, bfs_ids and samples."""
    cases = []
    paths = sorted(glob.glob(os.path.join(GOLDEN, prefix + "_*.json")))
    assert paths, "no fixture files " + prefix
    for path in paths:
        by_name = {}
        for case in json.load(open(path))["cases"]:
            for r in case["results"]:                    # the sorted clade lists are stored as [name, count] runs
                for order in ("asc", "desc"):
                    place = r[order]["place"]
                    if "clades_rle" in place:
                        place["clades"] = [[best, [nm for nm, k in runs for _ in range(k)]] for best, runs in place.pop("clades_rle")]
            if "same_tree_as" in case:
                base = by_name[case["same_tree_as"]]
                case = dict(case, tree=base["tree"], bfs_ids=base["bfs_ids"], lists=False, clades_only=True)
                for r, b in zip(case["results"], base["results"]):
                    r["sample"] = b["sample"]
                    for order in ("asc", "desc"):
                        place = dict(b[order]["place"])
                        place["clades"] = r[order]["place"]["clades"]
                        r[order] = dict(place=place)
            by_name[case["name"]] = case
            cases.append(case)
    return cases


def tree_of(case):
    t = case["tree"]
    return Tree(t["parent"], t["mut_off"], t["mut_pos"], t["mut_ref"], t["mut_mut"], t["mut_par"])


def samples_of(case):
    return [[tuple(e) for e in r["sample"]] for r in case["results"]]


def columns_of(sample):
    """(positions, refs, muts, missing) of one sample"""
    return tuple(list(c) for c in zip(*sample)) if sample else ([], [], [], [])


def root_masked_kinds(case):
    """(zeroed, non-zero): whether the root carries a masked mutation as the .pb loader leaves it / one with
    ref_nuc != mut_nuc, the kind that costs the root one and that the reference lists (usher_mapper.cpp:426-445)"""
    t = case["tree"]
    root = t["parent"].index(-1)
    zeroed = nonzero = False
    for k in range(t["mut_off"][root], t["mut_off"][root + 1]):
        if t["mut_pos"][k] < 0:
            if t["mut_ref"][k] != t["mut_mut"][k]:
                nonzero = True
            elif not (t["mut_ref"][k] or t["mut_par"][k] or t["mut_mut"][k]):
                zeroed = True
    return zeroed, nonzero


def excess_digest(lists):
    """The driver's "excess_listed" of one sample from its per-node excess lists [(position, ref, par, mut)] in BFS
    order: FNV-1a over 32-bit words, per node the length and then the four fields of every entry."""
    h = 1469598103934665603
    for entries in lists:
        for w in [len(entries)] + [x for e in entries for x in e]:
            h = ((h ^ (int(w) & 0xFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return str(h)
