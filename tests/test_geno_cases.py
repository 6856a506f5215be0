"""Every input of tests/geno_cases.py held to the edge it is named for, on the CPU: what the GPU and the emulation
tests run is what the layout constants of wepp_amd/csrc/geno.hpp call for."""
import numpy as np

import geno_cases as gc
import geno_model as gm

CASES = {c["name"]: c for c in gc.cases()}


def sizes(c):
    return np.diff(c["grp_off"].astype(np.int64)).tolist()


def columns(c, k):
    lo, hi = int(c["grp_off"][k]), int(c["grp_off"][k + 1])
    return len(set(p for g in c["items"][lo:hi] for p, _, _ in g))


def test_constants_come_from_the_header():
    assert gc.WAVE_ITEMS == 64 and gc.TILE == 64 and gc.CHUNK_WORDS >= 1 and gc.PASS_BYTES == 1 << 30


def test_every_input_is_a_legal_genotype_list():
    for c in list(CASES.values()) + gc.fuzz(3, 10):
        for g in c["items"]:
            pos = [p for p, _, _ in g]
            assert pos == sorted(set(pos)) and all(0 <= p <= gc.MAX_POSITION for p in pos)
            assert all(m != r and 1 <= m <= 15 for _, r, m in g)


def test_group_sizes():
    assert sizes(CASES["sizes"]) == [0, 1, 2, 63, 64, 65, 128, 129]
    want = gc.expected(CASES["sizes"])
    assert want[0] == 0 and want[1] == 0 and all(want[2:] > 0)


def test_group_mix():
    s = sizes(CASES["mix"])
    assert len(s) == 41 and s[17] == 129 and all(1 <= x <= 3 for i, x in enumerate(s) if i != 17)
    assert {1, 2, 3} <= set(s)


def test_column_counts():
    for name, n in (("columns_wave", 3), ("columns_tile", 65)):
        c = CASES[name]
        assert sizes(c) == [n] * 6
        assert [columns(c, k) for k in range(6)] == [0, 1, 63, 64, 65, 129]
    # ... and more than one LDS chunk of column words, the second one partly filled
    c = CASES["columns_two_chunks"]
    assert sizes(c) == [65, 2] and columns(c, 0) == columns(c, 1) == 64 * gc.CHUNK_WORDS + 1
    c = CASES["near_two_chunks"]
    assert len(set(p for g in c["items"] for p, _, _ in g)) == 64 * gc.CHUNK_WORDS + 1 and len(c["items"]) - c["n_a"] == 65


def test_position_extremes():
    c = CASES["extremes"]
    pos = set(p for g in c["items"] for p, _, _ in g)
    assert 1 in pos and gc.MAX_POSITION in pos and sizes(c) == [3, 65]


def test_keep_mask_cuts_inside_a_word():
    c = CASES["keep_cut"]
    assert c["keep_positions"] % 32 != 0 and any(p >= c["keep_positions"] for p in c["keep"])
    assert any(p >= c["keep_positions"] for g in c["items"] for p, _, _ in g)
    assert 44 in c["keep"]                      # the last position inside
    bits = gm.keep_bits(c["keep"], c["keep_positions"])
    assert bits.size == 2 and int(bits[1]) >> (c["keep_positions"] - 32) == 0
    assert gc.expected(c).tolist() != gm.diameters(c["items"], c["grp_off"]).tolist()    # the mask matters
    assert gc.expected(CASES["keep_none_left"]).tolist() == [0, 0]


def test_passes():
    assert len(gc.plan_passes(CASES["sizes"])) == 1
    assert len(gc.plan_passes(CASES["sizes_two_passes"])) == 2
    per = gc.plan_passes(CASES["sizes_pass_per_group"])
    big = [sum(1 for k in p if sizes(CASES["sizes"])[k] >= 2) for p in per]
    assert max(big) == 1 and sum(big) == 6      # (groups of fewer than two items take no planes: they join any pass)
    assert sum(len(p) for p in per) == 8
    per = gc.plan_passes(CASES["mix_pass_per_group"])
    assert max(sum(1 for k in p if sizes(CASES["mix"])[k] >= 2) for p in per) == 1 and len(per) >= 20


def test_nearest_shapes():
    for na, nb in ((1, 1), (65, 1), (1, 65), (65, 129)):
        c = CASES["near_%dx%d" % (na, nb)]
        assert c["n_a"] == na and len(c["items"]) == na + nb


def test_ties_are_broken_across_tiles():
    c = CASES["near_ties"]
    md, nr, mat = gc.expected(c)
    assert md.tolist() == [0, 1] and nr.tolist() == [3, 100]
    assert np.flatnonzero(mat[0] == 0).tolist() == [3, 70] and 3 // gc.TILE != 70 // gc.TILE
    assert np.flatnonzero(mat[1] == 1).tolist() == [100, 128] and 100 // gc.TILE != 128 // gc.TILE
    md, nr, mat = gc.expected(CASES["near_keep_none_left"])
    assert not mat.any() and nr.tolist() == [0, 0, 0]
