"""geno_capi.cpp and the kernels of geno_kernels.hip under the CPU emulation (tests/geno_emu.py), unchanged: every
case of tests/geno_cases.py and the fuzz against the model, and every WEPP_EINVAL / WEPP_ELIMIT path with its message."""
import ctypes

import numpy as np
import pytest

import geno_cases as gc
import geno_emu
import geno_model as gm
import wepp_amd as w
from wepp_amd import _lib

CASES = gc.cases()
A, C, G = 1, 2, 4


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_equals_model(case):
    gc.check(case, gc.run(case, geno_emu.diameters, geno_emu.nearest))


def test_pass_variable_changes_no_result():
    for name in ("mix", "columns_tile", "keep_cut"):
        case = next(c for c in CASES if c["name"] == name)
        for pb in (None, 1, 4096):
            gc.check(case, gc.run(case, geno_emu.diameters, geno_emu.nearest, force_pass_bytes=pb))


def test_fuzz_equals_model():
    for case in gc.fuzz(99, 40):
        gc.check(case, gc.run(case, geno_emu.diameters, geno_emu.nearest))


def word(p, r, m, extra=0):
    return int(w.pack_read_word(p, r, m)) | extra


def fails(code, text, fn, *args, **kw):
    with pytest.raises(w.WeppError) as e:
        fn(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_invalid_genotypes():
    d, n = geno_emu.diameters, geno_emu.nearest
    one = np.array([0, 1], np.uint64)
    grp = np.array([0, 1], np.uint32)
    fails(1, "positions are not strictly ascending", d, np.array([0, 2], np.uint64), np.array([word(5, A, C), word(4, A, C)], np.uint32), grp)
    fails(1, "item 0, word 1: positions are not strictly ascending", d, np.array([0, 2], np.uint64),
          np.array([word(5, A, C), word(5, A, G)], np.uint32), grp)
    fails(1, "mut_nuc equals ref_nuc", d, one, np.array([word(5, A, A)], np.uint32), grp)
    fails(1, "mut_nuc is 0", d, one, np.array([word(5, A, 0)], np.uint32), grp)
    fails(1, "position exceeds WEPP_MAX_POSITION", d, one, np.array([word(0xFFFFF, A, C)], np.uint32), grp)
    fails(1, "bits above mut_nuc are set", d, one, np.array([word(5, A, C, 1 << 28)], np.uint32), grp)
    fails(1, "item_off does not ascend at item 1", d, np.array([0, 1, 0], np.uint64), np.array([word(5, A, C)], np.uint32), np.array([0, 2], np.uint32))
    fails(1, "item_off[0] is not 0", d, np.array([1, 1], np.uint64), np.array([word(5, A, C)], np.uint32), grp)
    fails(1, "mut_nuc is 0", n, np.array([0, 1, 1], np.uint64), np.array([word(5, A, 0)], np.uint32), 1)


def test_invalid_groups_and_sides():
    d, n = geno_emu.diameters, geno_emu.nearest
    off, words = np.array([0, 1, 1, 2], np.uint64), np.array([word(5, A, C), word(6, C, G)], np.uint32)
    fails(1, "grp_off ends at 2, not at n_items = 3", d, off, words, np.array([0, 2], np.uint32))
    fails(1, "grp_off does not ascend at group 1", d, off, words, np.array([0, 2, 1, 3], np.uint32))
    fails(1, "grp_off[0] is not 0", d, off, words, np.array([1, 3], np.uint32))
    fails(1, "A is empty", n, off, words, 0)
    fails(1, "B is empty", n, off, words, 3)
    assert d(off, words, np.array([0, 3], np.uint32)).tolist() == [2]      # the same input, legal


def test_null_arguments():
    L = geno_emu.lib()
    off, grp = np.zeros(2, np.uint64), np.array([0, 1], np.uint32)
    g = _lib.GenotypesC(1, off.ctypes.data, None)
    out = np.zeros(1, np.int32)
    assert L.wepp_geno_diameters(0, None, None, 0, 1, grp.ctypes.data, out.ctypes.data) == 1
    assert L.wepp_last_error() == b"null argument"
    assert L.wepp_geno_diameters(0, ctypes.byref(g), None, 0, 1, None, out.ctypes.data) == 1
    assert L.wepp_geno_diameters(0, ctypes.byref(g), None, 0, 1, grp.ctypes.data, None) == 1
    assert L.wepp_geno_diameters(0, ctypes.byref(_lib.GenotypesC(1, None, None)), None, 0, 1, grp.ctypes.data, out.ctypes.data) == 1
    assert L.wepp_geno_nearest(0, ctypes.byref(g), 1, None, 0, None, out.ctypes.data, None) == 1
    assert L.wepp_geno_nearest(0, ctypes.byref(g), 1, None, 0, out.ctypes.data, None, None) == 1
    assert L.wepp_last_error() == b"null argument"
    off2 = np.array([0, 1], np.uint64)      # a word is announced, item_word is null
    assert L.wepp_geno_diameters(0, ctypes.byref(_lib.GenotypesC(1, off2.ctypes.data, None)), None, 0, 1, grp.ctypes.data, out.ctypes.data) == 1


def test_limits():
    L = geno_emu.lib()
    out = np.zeros(1, np.int32)
    off = np.zeros(2, np.uint64)
    grp = np.array([0, 1], np.uint32)
    assert L.wepp_geno_diameters(0, ctypes.byref(_lib.GenotypesC(1 << 31, off.ctypes.data, None)), None, 0, 1, grp.ctypes.data, out.ctypes.data) == 4
    assert L.wepp_last_error() == b"2^31 or more items in one call"
    off = np.array([0, 1 << 32], np.uint64)
    assert L.wepp_geno_diameters(0, ctypes.byref(_lib.GenotypesC(1, off.ctypes.data, None)), None, 0, 1, grp.ctypes.data, out.ctypes.data) == 4
    assert L.wepp_last_error() == b"2^32 or more words in one call"
    # a matrix beyond 2^28 cells: 2^14 + 1 items of A against 2^14 of B, all empty (refused before any work)
    n_a, n_b = (1 << 14) + 1, 1 << 14
    off = np.zeros(n_a + n_b + 1, np.uint64)
    md, nr = np.zeros(n_a, np.int32), np.zeros(n_a, np.uint32)
    g = _lib.GenotypesC(n_a + n_b, off.ctypes.data, None)
    assert L.wepp_geno_nearest(0, ctypes.byref(g), n_a, None, 0, md.ctypes.data, nr.ctypes.data, md.ctypes.data) == 4
    assert b"cells exceeds 2^28" in L.wepp_last_error()
    # a single group beyond the pass bound: 2^17 items of two entries each, 2^18 distinct columns -> 4096 words
    # x 32 bytes x 2^17 items = 16 GiB of planes (the column phase runs; no plane is made)
    n = 1 << 17
    pos = np.arange(1, 2 * n + 1, dtype=np.uint32)
    words = (pos | (np.uint32(1 << (0)) << np.uint32(20)) | (np.uint32(2) << np.uint32(24))).astype(np.uint32)
    off = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    with pytest.raises(w.WeppError) as e:
        geno_emu.diameters(off, words, np.array([0, n], np.uint32))
    assert e.value.code == 4 and "more than a pass holds" in str(e.value) and "group 0 (131072 items, 262144 columns)" in str(e.value)


def test_legal_corners():
    d = geno_emu.diameters
    assert d(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint32)).size == 0          # no groups
    assert d(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.array([0, 0, 1, 2, 2], np.uint32)).tolist() == [0, 0, 0, 0]
    assert d(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.array([0, 2], np.uint32)).tolist() == [0]   # empty genotypes
    off, words = gm.pack([[(0, A, C)], [(0, A, G)]])                                                   # position 0 is a position
    assert d(off, words, np.array([0, 2], np.uint32)).tolist() == [1]
