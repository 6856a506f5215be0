"""Small inputs for wepp_geno_diameters / wepp_geno_nearest, one per edge of the device layout (tests/test_geno_cases.py
holds each to its edge on the CPU; tests/test_geno_emulation.py and tests/test_geno_gpu.py run them).  The wave and
tile constants are read from wepp_amd/csrc/geno.hpp, so a case follows the kernels when they change.

A case is a dict: kind "diam" (items, grp_off) or "near" (items, n_a); keep = a set of positions or None with
keep_positions; pass_bytes = the value of WEPP_GENO_PASS_BYTES for the call or None."""
import contextlib
import functools
import os
import re

import numpy as np

import fuzz_trees
import geno_model

_HPP = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "wepp_amd", "csrc", "geno.hpp")).read()


def _const(name):
    m = re.search(r"constexpr\s+uint(?:32|64)_t\s+%s\s*=\s*([^;]+);" % name, _HPP)
    assert m, name + " is not in geno.hpp"
    return int(eval(re.sub(r"(\d+)u(ll)?\b", r"\1", m.group(1)), {"GENO_TILE": 64}))


WAVE_ITEMS = _const("GENO_WAVE_ITEMS")     # groups up to this size take one wave
TILE = _const("GENO_TILE")                 # items per side of a tile
CHUNK_WORDS = _const("GENO_CHUNK_WORDS")   # 64-bit column words per LDS chunk
PASS_BYTES = _const("GENO_PASS_BYTES")
MAX_POSITION = 0xFFFFE                     # WEPP_MAX_POSITION (include/wepp_place.h)
assert WAVE_ITEMS == TILE == 64, "the sizes below are written for waves and tiles of 64 items"


def ref_of(p):
    return 1 << (p % 4)


def make_group(rng, n, positions):
    """n items over exactly the given positions: every position is held by at least one item (when n > 0)"""
    items = []
    for i in range(n):
        g = []
        for j, p in enumerate(positions):
            if j % n == i or rng.random() < 0.4:
                m = int(rng.integers(1, 16))
                while m == ref_of(p):
                    m = int(rng.integers(1, 16))
                g.append((p, ref_of(p), m))
        items.append(g)
    return items


def _positions(rng, count, lo=1, hi=400):
    return sorted(int(x) for x in rng.choice(np.arange(lo, hi + 1), size=count, replace=False))


def _diam(name, groups, **kw):
    items, off = [], [0]
    for g in groups:
        items += g
        off.append(len(items))
    return dict(name=name, kind="diam", items=items, grp_off=np.array(off, np.uint32), keep=kw.get("keep"),
                keep_positions=kw.get("keep_positions", 0), pass_bytes=kw.get("pass_bytes"))


def _near(name, A, B, **kw):
    return dict(name=name, kind="near", items=A + B, n_a=len(A), keep=kw.get("keep"), keep_positions=kw.get("keep_positions", 0),
                pass_bytes=kw.get("pass_bytes"))


GROUP_SIZES = [0, 1, 2, WAVE_ITEMS - 1, WAVE_ITEMS, WAVE_ITEMS + 1, 2 * TILE, 2 * TILE + 1]
COLUMN_COUNTS = [0, 1, 63, 64, 65, 64 * CHUNK_WORDS // 2 + 1]      # 129 with chunks of 4 words: one word into the next 64-bit word


def group_plane_bytes(case, k):
    """the bytes of planes group k takes on the device: items x ceil(kept columns / 64) x 4 planes x 8 bytes; groups of
    fewer than two items take none"""
    lo, hi = int(case["grp_off"][k]), int(case["grp_off"][k + 1])
    if hi - lo < 2:
        return 0
    cols = set(p for g in case["items"][lo:hi] for p, _, _ in geno_model.keep_only(g, case["keep"]))
    return (hi - lo) * ((len(cols) + 63) // 64) * 32


def plan_passes(case):
    """the pass rule of geno_capi.cpp restated: consecutive groups while their planes fit the bound, at least one"""
    bound = min(case["pass_bytes"] or PASS_BYTES, PASS_BYTES)
    passes, cur, used = [], [], 0
    for k in range(len(case["grp_off"]) - 1):
        b = group_plane_bytes(case, k)
        if cur and used + b > bound:
            passes.append(cur); cur, used = [], 0
        cur.append(k); used += b
    return passes + ([cur] if cur else [])


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261020)
    out = []
    sizes = [make_group(rng, n, _positions(rng, 70)) for n in GROUP_SIZES]
    out.append(_diam("sizes", sizes))
    # passes: the same call cut in two, and one group (of two items or more) per pass
    total = sum(group_plane_bytes(out[0], k) for k in range(len(GROUP_SIZES)))
    out.append(_diam("sizes_two_passes", sizes, pass_bytes=total - 1))
    out.append(_diam("sizes_pass_per_group", sizes, pass_bytes=1))
    # many tiny groups beside one of two tiles and an item
    mix = [make_group(rng, int(rng.integers(1, 4)), _positions(rng, 5)) for _ in range(40)]
    mix.insert(17, make_group(rng, 2 * TILE + 1, _positions(rng, 40)))
    out.append(_diam("mix", mix))
    out.append(_diam("mix_pass_per_group", mix, pass_bytes=1))
    # column counts, in the wave form (3 items) and in the tile form (65 items)
    out.append(_diam("columns_wave", [make_group(rng, 3, _positions(rng, c)) for c in COLUMN_COUNTS]))
    out.append(_diam("columns_tile", [make_group(rng, TILE + 1, _positions(rng, c)) for c in COLUMN_COUNTS]))
    # the two ends of the position range
    ext = [1, 2, MAX_POSITION - 1, MAX_POSITION]
    out.append(_diam("extremes", [make_group(rng, 3, ext), make_group(rng, TILE + 1, ext)]))
    # a keep mask whose keep_positions cuts inside a 32-bit word of keep_bits: positions 45 .. 100 are dropped
    pos = list(range(1, 101))
    keep = set(int(p) for p in pos if rng.random() < 0.6) | {44}
    out.append(_diam("keep_cut", [make_group(rng, 5, pos), make_group(rng, TILE + 6, pos)], keep=keep, keep_positions=45))
    out.append(_diam("keep_none_left", [make_group(rng, 4, pos), make_group(rng, TILE + 1, pos)], keep=set(), keep_positions=200))
    out.append(_diam("no_groups", []))
    out.append(_diam("empty_genotypes", [[[], [], []], [[]] * (TILE + 1)]))
    # A x B
    P = _positions(rng, 90)
    for na, nb in ((1, 1), (TILE + 1, 1), (1, TILE + 1), (TILE + 1, 2 * TILE + 1)):
        g = make_group(rng, na + nb, P)
        out.append(_near("near_%dx%d" % (na, nb), g[:na], g[na:]))
    # ties across tiles: a0 equals b3 and b70 (tiles 0 and 1); a1 is one step from b100 and b128 (tiles 1 and 2) only
    B = make_group(rng, 2 * TILE + 1, P)
    B[70] = list(B[3])
    far = [(p, ref_of(p), 15 if ref_of(p) != 15 else 7) for p in range(1000, 1040)]     # 40 entries nobody else holds
    B[100] = far + [(2000, ref_of(2000), 15)]
    B[128] = far + [(2001, ref_of(2001), 15)]
    out.append(_near("near_ties", [list(B[3]), list(far)], B))
    out.append(_near("near_keep_none_left", make_group(rng, 3, P), make_group(rng, TILE + 1, P), keep=set(), keep_positions=64))
    keep = set(P[::2])
    out.append(_near("near_keep_cut", make_group(rng, 5, P), make_group(rng, TILE + 2, P), keep=keep, keep_positions=P[50] + 1))
    # more columns than one LDS chunk holds: the tile kernel's second, partly filled chunk
    Q = _positions(rng, 64 * CHUNK_WORDS + 1, hi=3000)
    out.append(_diam("columns_two_chunks", [make_group(rng, TILE + 1, Q), make_group(rng, 2, Q)]))
    g = make_group(rng, 3 + TILE + 1, Q)
    out.append(_near("near_two_chunks", g[:3], g[3:]))
    return out


def fuzz(seed, n_trees):
    """cases over the genotypes of fuzz trees: random groups of random nodes, and a random split into A and B"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n_trees):
        tree, _ = fuzz_trees.random_tree(rng, n_nodes=int(rng.integers(2, 90)))
        genos = [geno_model.get_mutations(tree, n) for n in range(tree.n_nodes)]
        keep = None if rng.random() < 0.5 else set(int(p) for p in range(1, 61) if rng.random() < 0.7)
        kp = int(rng.integers(30, 70))
        groups = []
        for _ in range(int(rng.integers(1, 8))):
            groups.append([genos[int(i)] for i in rng.integers(0, tree.n_nodes, size=int(rng.integers(0, 12)))])
        if t % 8 == 0:
            groups.append([genos[int(i)] for i in rng.integers(0, tree.n_nodes, size=TILE + 3)])
        out.append(_diam("fuzz%d_diam" % t, groups, keep=keep, keep_positions=kp, pass_bytes=None if t % 2 else 64))
        A = [genos[int(i)] for i in rng.integers(0, tree.n_nodes, size=int(rng.integers(1, 9)))]
        B = [genos[int(i)] for i in rng.integers(0, tree.n_nodes, size=int(rng.integers(1, 20)))]
        out.append(_near("fuzz%d_near" % t, A, B, keep=keep, keep_positions=kp))
    return out


_EXPECTED = {}


def expected(case):
    """the model's answer, computed once per case and process"""
    if case["name"] not in _EXPECTED:
        keep = None if case["keep"] is None else set(p for p in case["keep"] if p < case["keep_positions"])
        if case["kind"] == "diam":
            _EXPECTED[case["name"]] = geno_model.diameters(case["items"], case["grp_off"], keep)
        else:
            _EXPECTED[case["name"]] = geno_model.nearest(case["items"], case["n_a"], keep)
    return _EXPECTED[case["name"]]


@contextlib.contextmanager
def pass_bytes(value):
    old = os.environ.pop("WEPP_GENO_PASS_BYTES", None)
    if value is not None:
        os.environ["WEPP_GENO_PASS_BYTES"] = str(value)
    try:
        yield
    finally:
        os.environ.pop("WEPP_GENO_PASS_BYTES", None)
        if old is not None:
            os.environ["WEPP_GENO_PASS_BYTES"] = old


def run(case, diameters, nearest, force_pass_bytes="case"):
    """the case through the given entry points (signatures of wepp_amd.geno_diameters / geno_nearest)"""
    off, words = geno_model.pack(case["items"])
    kb = None if case["keep"] is None else geno_model.keep_bits(case["keep"], case["keep_positions"])
    with pass_bytes(case["pass_bytes"] if force_pass_bytes == "case" else force_pass_bytes):
        if case["kind"] == "diam":
            return diameters(off, words, case["grp_off"], kb, case["keep_positions"])
        return nearest(off, words, case["n_a"], kb, case["keep_positions"], want_matrix=True)


def check(case, got):
    want = expected(case)
    if case["kind"] == "diam":
        assert got.tolist() == want.tolist(), case["name"]
    else:
        assert got[0].tolist() == want[0].tolist(), case["name"] + ": min_dist"
        assert got[1].tolist() == want[1].tolist(), case["name"] + ": nearest"
        assert got[2].tolist() == want[2].tolist(), case["name"] + ": matrix"
