"""ctypes binding of wepp_geno_diameters / wepp_geno_nearest (include/wepp_place.h): pairwise distances between
genotypes given as lists of packed words.  Computes nothing itself."""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, check
from .api import _ptr


def pack_genotypes(items):
    """items: one array of packed words (pack_read_word(pos, ref, mut)) per item -> (item_off uint64, item_word uint32)"""
    off = np.zeros(len(items) + 1, np.uint64)
    if len(items):
        off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    words = np.concatenate([np.asarray(x, np.uint32).ravel() for x in items]) if len(items) else np.zeros(0, np.uint32)
    return off, np.ascontiguousarray(words, np.uint32)


def _genotypes(item_off, item_word):
    item_off = np.ascontiguousarray(item_off, np.uint64)
    item_word = np.ascontiguousarray(item_word, np.uint32)
    g = _lib.GenotypesC(int(item_off.size) - 1, _ptr(item_off).value, _ptr(item_word).value if item_word.size else None)
    return g, (item_off, item_word)


def _keep(keep_bits, keep_positions):
    if keep_bits is None:
        return None, 0, None
    kb = np.ascontiguousarray(keep_bits, np.uint32)
    kb = kb if kb.size else np.zeros(1, np.uint32)
    return _ptr(kb).value, int(keep_positions), kb


def geno_diameters(item_off, item_word, grp_off, keep_bits=None, keep_positions=0, device=0, call=None):
    """wepp_geno_diameters: diam[n_groups] int32.  `call` replaces the library's entry point (the emulation's)."""
    g, alive = _genotypes(item_off, item_word)
    grp_off = np.ascontiguousarray(grp_off, np.uint32)
    n_groups = int(grp_off.size) - 1
    diam = np.full(max(n_groups, 1), -7, np.int32)
    kp, kn, kalive = _keep(keep_bits, keep_positions)
    fn = call or (lambda *a: check(lib.wepp_geno_diameters(*a)))
    fn(int(device), ctypes.byref(g), kp, kn, n_groups, _ptr(grp_off).value, _ptr(diam).value)
    return diam[:n_groups]


def geno_nearest(item_off, item_word, n_a, keep_bits=None, keep_positions=0, device=0, want_matrix=False, call=None):
    """wepp_geno_nearest: (min_dist[n_a] int32, nearest[n_a] uint32, matrix[n_a, n_b] int32 or None)"""
    g, alive = _genotypes(item_off, item_word)
    n_a = int(n_a)
    n_b = max(g.n_items - n_a, 0)
    md = np.full(max(n_a, 1), -7, np.int32)
    nr = np.full(max(n_a, 1), 0xFFFFFFFF, np.uint32)
    mat = np.full((n_a, n_b), -7, np.int32) if want_matrix else None
    kp, kn, kalive = _keep(keep_bits, keep_positions)
    fn = call or (lambda *a: check(lib.wepp_geno_nearest(*a)))
    fn(int(device), ctypes.byref(g), n_a, kp, kn, _ptr(md).value, _ptr(nr).value, _ptr(mat).value if want_matrix and mat.size else None)
    return md[:n_a], nr[:n_a], mat


def geno_last_timing():
    """device ms of the calling thread's last geno call: columns, planes, pairs"""
    v = [ctypes.c_double() for _ in range(3)]
    check(lib.wepp_geno_last_timing(*[ctypes.byref(x) for x in v]))
    return dict(zip(("columns_ms", "planes_ms", "pairs_ms"), (x.value for x in v)))
