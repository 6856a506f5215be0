"""The model of wepp_epp_neighbors (tests/neighbors_model.py) itself: its distances against the oracle's
haplotype::mutation_distance, its regions against their definition (the connected component of the pivot among
the nodes within the radius) and by hand, and that the fuzz the GPU test runs is not vacuous."""
import numpy as np
import pytest

import neighbors_model as nm
import wepp_amd as w

TO, FROM = nm.TO, nm.FROM


def _as_read(ar, k):
    s = ar.stack[k]
    return [p for p, _ in s], [ar.ref[p] for p, _ in s], [m for _, m in s]


def test_distances_are_the_oracles(oracle):
    for it, (tree, ar, piv) in enumerate(nm.fuzz_cases(12)):
        ot = oracle.OracleTree(tree)
        # form TO: node->mutation_distance(pivot), one call per pivot
        for p in piv:
            assert np.array_equal(ot.epp_distance(*_as_read(ar, int(p)), 0, nm.INT_MAX), ar.field(int(p), TO)), (it, p)
        # form FROM: pivot->mutation_distance(node), one call per node, the pivot's entry
        per_node = np.array([ot.epp_distance(*_as_read(ar, k), 0, nm.INT_MAX) for k in range(ar.n)], np.int32)
        for p in piv:
            assert np.array_equal(per_node[:, int(p)], ar.field(int(p), FROM)), (it, p)
        ot.close()


def test_forms_differ_only_through_n():
    seen = False
    for tree, ar, piv in nm.fuzz_cases(40):
        for p in piv:
            a, b = ar.field(int(p), TO), ar.field(int(p), FROM)
            has_n = [any(m == 15 for _, m in s) for s in ar.stack]
            same = a == b
            assert all(same[k] or has_n[k] or has_n[int(p)] for k in range(ar.n))
            seen |= not same.all()
    assert seen


def _component(ar, piv, ok):
    comp, todo = set(), [piv]
    while todo:
        x = todo.pop()
        if x in comp or not ok[x]:
            continue
        comp.add(x)
        todo += ar.children[x] + ([ar.parent[x]] if ar.parent[x] >= 0 else [])
    return comp


def test_regions_are_components_and_the_fuzz_is_not_vacuous():
    """both traversals list the pivot's component of {n : D(n) <= R}; at least a third of the regions of the fuzz
    of tests/test_epp_neighbors_gpu.py are neither the pivot alone nor the whole tree"""
    total = partial = 0
    for tree, ar, piv in nm.fuzz_cases():
        for form in (TO, FROM):
            for p in piv:
                D = ar.field(int(p), form)
                for R in nm.FUZZ_RADII:
                    reg = ar.region(int(p), R, form)
                    assert set(reg) == _component(ar, int(p), D <= R)
                    assert all(reg[k] == D[k] for k in reg)
                    total += 1
                    partial += 1 < len(reg) < ar.n
    assert 3 * partial >= total, (partial, total)


@pytest.mark.parametrize("name", sorted(nm.hand_cases()))
def test_hand_cases(name):
    tree, piv, radius, skip, want = nm.hand_cases()[name]
    ar = nm.Arena(tree)
    for form in (TO, FROM):
        got = ar.neighbors(piv, radius, form, skip)
        lists = [got["nbr_node"][int(got["nbr_off"][i]):int(got["nbr_off"][i + 1])].tolist() for i in range(len(piv))]
        assert lists == want[form], (name, form)


def test_radius_zero_and_radius_beyond_every_distance():
    tree, ar, piv = next(nm.fuzz_cases(1, seed=5))
    for form in (TO, FROM):
        whole = ar.neighbors(piv, 10**6, form)
        assert (whole["n_region"] == ar.n).all() and (whole["top"] == 0).all()
        assert np.array_equal(whole["nbr_node"], np.tile(np.arange(ar.n, dtype=np.uint32), len(piv)))
        zero = ar.neighbors(piv, 0, form)
        assert (zero["nbr_dist"] == 0).all() and (zero["n_region"] >= 1).all()
        for i, p in enumerate(piv):
            assert int(p) in zero["nbr_node"][int(zero["nbr_off"][i]):int(zero["nbr_off"][i + 1])]
