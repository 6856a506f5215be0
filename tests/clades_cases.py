"""Trees, samples and annotation patterns for the clade tests (tests/test_clades_gpu.py, tests/test_host_clades.py,
tools/diag/clades_probe.py), and the expected result of a batch from the oracle's optimal nodes and
tests/clades_model.py."""
import numpy as np

import clades_model as cm
from wepp_amd import Reads, Tree, number_clade_names

A, C, G, T = 1, 2, 4, 8
SUBS = 5            # sub-parents per hub group
POOL = ["B.1", "B.1.1", "UNDEFINEE", "A", "20A"]   # names around "UNDEFINED" in the order, one a prefix of another


def hub_tree(sizes):
    """A root without mutations; the `probe` node (two mutations, one leaf child) whose has_unique depends on the
    sample; and one GROUP per entry of sizes: g (one mutation of its own) -> SUBS sub-parents without mutations ->
    sizes[i] leaves, dealt round-robin to the sub-parents, that all carry the group's second mutation.  A sample
    with the group's two mutations has exactly its leaves as optimal nodes.  Returns (Tree, info)."""
    parent, muts, kind = [-1], [[]], ["root"]

    def add(p, ml, k):
        parent.append(p); muts.append(ml); kind.append(k)
        return len(parent) - 1
    probe = add(0, [(5, A, A, C), (6, A, A, G)], "probe")
    add(probe, [(7, A, A, T)], "leaf")
    groups = []
    for i, h in enumerate(sizes):
        p_own, p_leaf = 10 + 2 * i, 11 + 2 * i
        g = add(0, [(p_own, A, A, C)], "group")
        subs = [add(g, [], "sub") for _ in range(SUBS)]
        for k in range(h):
            add(subs[(k * 7 + i) % SUBS], [(p_leaf, A, A, G)], "leaf")
        groups.append(dict(node=g, subs=subs, size=h, sample=[(p_own, A, C, 0), (p_leaf, A, G, 0)]))
    info = dict(kind=kind, probe=probe, groups=groups,
                probe_shared=[(5, A, C, 0), (6, A, G, 0)], probe_unique=[(5, A, C, 0)])
    return Tree.from_lists(parent, muts), info


def annotate(kind, parent, n_columns, pattern, rng):
    """columns[c][node]: 'none', 'root', 'all' or 'mixed' (random names on a random part of the nodes, every leaf
    annotated so that a leaf's own clade, which must not be used, is always there to be used by mistake)."""
    n = len(kind)
    cols = []
    for c in range(n_columns):
        if pattern == "none":
            col = [""] * n
        elif pattern == "root":
            col = ["R%d" % c if parent[i] < 0 else "" for i in range(n)]
        elif pattern == "all":
            col = ["%s.%d" % (POOL[(i + c) % len(POOL)], i % 7) for i in range(n)]
        else:
            col = []
            for i in range(n):
                if kind[i] == "leaf":
                    col.append("LEAF.%d" % (i % 3))
                elif kind[i] == "probe":
                    col.append("PROBE")
                elif kind[i] == "root":
                    col.append("ROOT" if c % 2 == 0 else "")
                else:
                    col.append(POOL[int(rng.integers(0, len(POOL)))] if rng.random() < 0.6 else "")
        cols.append(col)
    return cols


def oracle_best(ot, samples):
    """Per sample the oracle's (best_j, num_best, ascending best_j_vec)."""
    out = []
    for s in samples:
        want = ot.place_sample([e[0] for e in s], [e[1] for e in s], [e[2] for e in s], [e[3] for e in s], want_best_vec=True)
        out.append((int(want["best_j"]), int(want["num_best"]), [int(x) for x in want["best_j_vec"]]))
    return out


def expected(tree, columns, samples, best):
    """(best_clade, hist_off, hist_clade, hist_count, per-sample model output, pairs) for the batch."""
    parent, muts = cm.tree_lists(tree)
    bfs, kids = cm.bfs_order(parent)
    _, _, names = number_clade_names(columns)
    name_ids = [{nm: i + 1 for i, nm in enumerate(col)} for col in names]
    per_sample, pairs = [], []
    for s, (bj, _nb, vec) in zip(samples, best):
        out, pr = cm.assign_sample(parent, kids, muts, bfs, columns, s, vec, bj)
        per_sample.append(out)
        pairs.append(pr)
    return cm.expected_arrays(per_sample, name_ids) + (per_sample, pairs)


def reads_of(samples):
    return Reads.from_lists(samples)
