"""The literal model of the genotype distances (tests/geno_model.py): one hand case per rule of include/wepp_place.h's
section on pairwise genotype distances, and a fuzz over random trees against a direct dense-vector Hamming distance."""
import numpy as np

import fuzz_trees
import geno_model as gm
import wepp_amd as w

A, C, G, T = 1, 2, 4, 8


def tree(parent, muts):
    return w.Tree.from_lists(parent, muts)


def test_two_alleles_at_one_site_count_once():
    assert gm.distance([(5, A, C)], [(5, A, G)]) == 1
    assert gm.distance([(5, A, C)], [(5, A, C)]) == 0
    assert gm.distance([(5, A, C)], []) == 1 and gm.distance([], [(5, A, C)]) == 1
    assert gm.distance([(5, A, C), (9, C, T)], [(7, G, A)]) == 3


def test_masks_are_compared_for_equality():
    # an ambiguous mask that contains the other allele is still another value; so is 15
    assert gm.distance([(5, A, C | G)], [(5, A, C)]) == 1
    assert gm.distance([(5, A, 15)], [(5, A, C)]) == 1
    assert gm.distance([(5, A, 15)], [(5, A, 15)]) == 0


def test_deepest_mutation_wins_and_back_mutation_removes_the_entry():
    # 0 -(5: A>C)- 1 -(5: C>A back)- 2 ; 1 -(5: C>G, 7: G>T)- 3
    t = tree([-1, 0, 1, 1], [[], [(5, A, A, C)], [(5, A, C, A)], [(5, A, C, G), (7, G, G, T)]])
    assert gm.get_mutations(t, 0) == []
    assert gm.get_mutations(t, 1) == [(5, A, C)]
    assert gm.get_mutations(t, 2) == []                       # back to the reference: no entry
    assert gm.get_mutations(t, 3) == [(5, A, G), (7, G, T)]   # the node's own mutation, not the ancestor's
    assert gm.distance(gm.get_mutations(t, 2), gm.get_mutations(t, 1)) == 1


def test_masked_mutation_is_ignored():
    t = tree([-1, 0], [[(-1, 0, 0, 0)], [(-1, 0, 0, 0), (3, C, C, T)]])
    assert gm.get_mutations(t, 0) == [] and gm.get_mutations(t, 1) == [(3, C, T)]


def test_empty_genotypes_and_groups():
    assert gm.distance([], []) == 0
    assert gm.diameters([[], [(1, A, C)], []], [0, 0, 1, 3]).tolist() == [0, 0, 1]


def test_keep_mask_can_empty_both_sides():
    a, b = [(5, A, C), (9, C, T)], [(7, G, A)]
    assert gm.diameters([a, b], [0, 2], keep=set()).tolist() == [0]
    assert gm.diameters([a, b], [0, 2], keep={9}).tolist() == [1]
    md, nr, mat = gm.nearest([a, b, a], 1, keep=set())
    assert md.tolist() == [0] and nr.tolist() == [0] and mat.tolist() == [[0, 0]]


def test_first_of_tied_nearest_wins():
    a = [(5, A, C)]
    md, nr, mat = gm.nearest([a, [(5, A, G)], [], a, a], 1)
    assert mat.tolist() == [[1, 1, 0, 0]] and md.tolist() == [0] and nr.tolist() == [2]
    md, nr, _ = gm.nearest([a, [(5, A, G)], []], 1)
    assert md.tolist() == [1] and nr.tolist() == [0]


def test_reports_formats():
    t = tree([-1, 0, 0], [[], [(2, C, C, T)], [(2, C, C, G), (4, A, A, T)]])
    ids = ["root", "x", "y"]
    assert gm.uncertainty_row(t, ids, [1]) == "0,x\n"
    assert gm.uncertainty_row(t, ids, [2, 1, 0]) == "2,y,x,root\n"
    lines, avg = gm.truth_lines(t, ids, [2, 0], [0, 1], keep={2})
    assert lines == ["* dist: 01 true_node: y pred_node: root \n", "* dist: 00 true_node: root pred_node: root \n"]
    assert "%0.3f" % avg == "0.500"
    assert gm.md_string(5, [(2, C, G), (4, A, T)]) == "MD:Z:1C1A1"
    assert gm.md_string(4, [(3, G, T), (4, A, T)]) == "MD:Z:2G0A"      # adjacent: a 0 between; no trailing 0
    assert gm.md_string(3, []) == "MD:Z:3"
    assert gm.haplotype_row("y", "ref", "ACGA", [(2, C, G), (4, A, T)]) == "y\t0\tref\t1\t60\t4M\t*\t0\t0\tAGGT\t????\tMD:Z:1C1A\tRG:Z:group\n"


def dense(tree, node, genome):
    """the genotype as a dense vector of masks, 0 = no entry: computed top-down, nothing shared with get_mutations"""
    path = []
    n = int(node)
    while n >= 0:
        path.append(n); n = int(tree.parent[n])
    cur, ref = {}, {}
    for n in reversed(path):
        for k in range(int(tree.mut_off[n]), int(tree.mut_off[n + 1])):
            if tree.mut_pos[k] >= 0:
                cur[int(tree.mut_pos[k])] = int(tree.mut_mut[k]); ref[int(tree.mut_pos[k])] = int(tree.mut_ref[k])
    v = np.zeros(genome + 1, np.int64)
    for p, m in cur.items():
        v[p] = m if m != ref[p] else 0
    return v


def test_fuzz_against_dense_hamming():
    rng = np.random.default_rng(7)
    for _ in range(60):
        t, _ = fuzz_trees.random_tree(rng)
        vec = [dense(t, n, 60) for n in range(t.n_nodes)]
        gen = [gm.get_mutations(t, n) for n in range(t.n_nodes)]
        for n in range(t.n_nodes):
            assert [p for p, _, _ in gen[n]] == np.flatnonzero(vec[n]).tolist()
        keep = set(int(p) for p in range(1, 61) if rng.random() < 0.6)
        kv = np.array([p in keep for p in range(61)])
        for _ in range(30):
            a, b = (int(x) for x in rng.integers(0, t.n_nodes, size=2))
            assert gm.distance(gen[a], gen[b]) == int((vec[a] != vec[b]).sum())
            assert gm.distance(gen[a], gen[b]) == gm.distance(gen[b], gen[a])
            assert gm.distance(gm.keep_only(gen[a], keep), gm.keep_only(gen[b], keep)) == int(((vec[a] != vec[b]) & kv).sum())
