"""Trees and VCF rows the Fitch-Sankoff kernels (fitch_kernels.hip, sort_reads.hip: launch_fitch_prepare) are built
around: polytomies at the 15-bit counter bound of the set forms, sibling groups at every offset of the 64-entry
parent vector, levels wider than a wave's chunk, spines at the depth bound of the LDS stack; rows that come unsorted,
name nodes twice, fill the mutation queue, or hold an empty allele set.

Every builder returns a Shape: a bare wepp_amd.Tree whose node ids are a seeded shuffle (the root is not id 0, parents
have larger ids than some of their children) and a preconditions() that asserts the property the shape exists for."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import fitch_model as fm
import oracle_bridge
import wepp_amd as w
from wepp_amd import A, C, G, T

NTHREADS = min(16, os.cpu_count() or 1)
LEVEL_CHUNK = 256            # fitch.hpp: FITCH_LEVEL_CHUNK
SETS_MAX_CHILDREN = 32767    # fitch.hpp: FITCH_SETS_MAX_CHILDREN
MAX_DEPTH = 140              # fitch.hpp: FITCH_MAX_DEPTH
FAN_COUNTS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)


class Shape:
    def __init__(self, name, parent, check, shuffled=True, **info):
        self.name = name
        parent = np.asarray(parent, np.int32)
        self.tree = w.Tree(parent, np.zeros(len(parent) + 1, np.uint32), [], [], [])
        self.topo = fm.Topology(parent)
        self._check = check
        self.shuffled = shuffled
        self.info = info

    def preconditions(self):
        t = self.topo
        if self.shuffled:
            root = int(np.flatnonzero(t.parent < 0)[0])
            assert root != 0, "the root must not be id 0"
            ids = np.arange(t.n)
            nonroot = ids[t.parent >= 0]
            assert (t.parent[nonroot] > nonroot).mean() > 0.2, "parents with larger ids than their children"
            assert (t.bfs2id != np.arange(t.n)).mean() > 0.9, "ids must not follow the BFS order"
        self._check(self)


class _Builder:
    """Nodes get their final ids from a seeded shuffle at creation; children of a node are ordered by ascending id, so a
    caller that needs a child at a given RANK among its siblings asks for all the sibling ids at once (sorted)."""

    def __init__(self, seed, n):
        rng = np.random.default_rng(seed)
        pool = rng.permutation(n)
        if pool[0] == 0:
            pool[[0, 1]] = pool[[1, 0]]
        self.pool, self.at, self.parent = pool, 0, np.full(n, -2, np.int64)

    def root(self):
        r = self.add(-1, 1)[0]
        return r

    def add(self, par, k):
        """k children of `par`, returned in sibling order (ascending id)"""
        ids = np.sort(self.pool[self.at:self.at + k])
        assert len(ids) == k, "node budget of the builder"
        self.at += k
        self.parent[ids] = par
        return ids

    def done(self):
        assert self.at == len(self.pool) and (self.parent > -2).all()
        return self.parent


def hub_ranks(k):
    """where the hub's internal children sit among its k children: first, last, around multiples of 64 and 256"""
    r = {0, 1, k - 2, k - 1}
    for m in (64, 128, 256, 512, 1024, 4096, (k // 256) * 256, (k // 256 - 1) * 256, (k // 64) * 64, (k // 2 // 256) * 256):
        r.update((m - 1, m, m + 1))
    return np.array(sorted(x for x in r if 0 <= x < k), np.int64)


def hub(k, seed=11):
    """root -> a hub with k children and a sibling leaf; a few dozen of the hub's children are internal: cherries, and
    chains of two unary nodes over a cherry, alternating."""
    ranks = hub_ranks(k)
    n_sub = sum(2 if i % 2 == 0 else 4 for i in range(len(ranks)))
    b = _Builder(seed, 3 + k + n_sub)
    root = b.root()
    # the hub takes the middle id: half of its children have smaller ids than their parent, half larger
    hub_id = len(b.pool) // 2
    at = int(np.flatnonzero(b.pool == hub_id)[0])
    if at == 0:
        hub_id += 1
        at = int(np.flatnonzero(b.pool == hub_id)[0])
    b.pool[[1, at]] = b.pool[[at, 1]]
    b.add(root, 2)
    kids = b.add(hub_id, k)
    for i, r in enumerate(ranks):
        x = int(kids[r])
        if i % 2:
            x = int(b.add(x, 1)[0])
            x = int(b.add(x, 1)[0])
        b.add(x, 2)

    def check(s):
        t = s.topo
        assert t.max_children == k, (t.max_children, k)
        assert t.n_children[hub_id] == k
        a, e = int(t.level_off[2]), int(t.level_off[3])
        assert e - a == k and (t.bfs2id[a:e] == kids).all(), "level 2 is the hub's children, in id order"
        internal = np.flatnonzero(~t.is_leaf_bfs[a:e])
        assert (internal == ranks).all() and len(ranks) >= 24, internal
        assert {0, k - 1, 63, 64, 65, 255, 256, 257} <= set(internal.tolist())
        assert t.max_depth == 5
    return Shape(f"hub{k}", b.done(), check, hub=hub_id, kids=kids, ranks=ranks)


def group_offsets(topo):
    """per sibling group: (start of the group - first child of its level chunk) mod 64, its length, and whether it crosses
    a 64-child window of that chunk's child stream (fitch_kernels.hip: pv in k_fitch_up)"""
    nc = topo.n_children[topo.bfs2id]
    coff = 1 + np.concatenate([[0], np.cumsum(nc)])
    res, length, cross = [], [], []
    for lev in range(len(topo.level_off) - 1):
        a, b = int(topo.level_off[lev]), int(topo.level_off[lev + 1])
        for ca in range(a, b, LEVEL_CHUNK):
            cb = min(b, ca + LEVEL_CHUNK)
            for p in range(ca, cb):
                if nc[p]:
                    s, e = int(coff[p] - coff[ca]), int(coff[p + 1] - coff[ca])
                    res.append(s % 64); length.append(e - s); cross.append(s // 64 != (e - 1) // 64)
    return np.array(res), np.array(length), np.array(cross)


def fans(seed=12):
    """Levels 1, 2 and 3 each hold nodes with every child count of FAN_COUNTS (in a seeded order, among leaves at seeded
    places), so that sibling groups begin at many offsets of the 64-entry parent vector and three levels are wider
    than a level chunk."""
    rng = np.random.default_rng(seed)
    tot = sum(FAN_COUNTS)
    passes2, passes3 = 5, 3
    n = 1 + len(FAN_COUNTS) + tot + passes2 * tot + passes3 * tot
    b = _Builder(seed, n)
    root = b.root()
    l1 = b.add(root, len(FAN_COUNTS))
    l2 = np.concatenate([b.add(int(p), int(c)) for p, c in zip(l1, rng.permutation(FAN_COUNTS))])
    # level 2: passes2 runs through the counts at seeded places, the other nodes stay leaves
    pick = rng.choice(len(l2), passes2 * len(FAN_COUNTS), replace=False)
    l3 = [b.add(int(l2[i]), int(c)) for i, c in zip(pick, np.concatenate([rng.permutation(FAN_COUNTS) for _ in range(passes2)]))]
    l3 = np.concatenate(l3)
    pick = rng.choice(len(l3), passes3 * len(FAN_COUNTS), replace=False)
    for i, c in zip(pick, np.concatenate([rng.permutation(FAN_COUNTS) for _ in range(passes3)])):
        b.add(int(l3[i]), int(c))

    def check(s):
        t = s.topo
        assert t.n == n and t.max_depth == 4
        assert (t.level_nodes > LEVEL_CHUNK).sum() >= 2, t.level_nodes
        depth = t.depth_of_ids()
        for lev in (1, 2, 3):
            assert set(FAN_COUNTS) <= set(t.n_children[depth == lev].tolist()), lev
        res, length, cross = group_offsets(t)
        assert len(set(res.tolist())) >= 32, sorted(set(res.tolist()))
        assert len(set((res % 16).tolist())) == 16
        assert (cross & (length >= 65)).any()
    return Shape("fans", b.done(), check)


def caterpillar(depth, unary=False, seed=13):
    """A spine of `depth` nodes with one leaf each, the last with two: the deepest nodes are `depth` edges below the root.
    unary = True: every third stretch of 5 spine nodes has no leaves (single children), and the last spine node has a
    bush of 360 leaves."""
    n_leafless = sum(1 for d in range(depth - 1) if unary and (d // 5) % 3 == 1)
    n = depth + (depth - 1 - n_leafless) + (2 if not unary else 300 + 60)
    b = _Builder(seed + depth + (1000 if unary else 0), n)
    x = b.root()
    for d in range(depth - 1):
        if unary and (d // 5) % 3 == 1:
            x = int(b.add(x, 1)[0])
        else:
            two = b.add(x, 2)
            x = int(two[d % 2])                  # the spine continues left or right of its leaf sibling
    if unary:
        b.add(x, 360)                            # the bush: one polytomy at the bottom of the stack
    else:
        b.add(x, 2)

    def check(s):
        t = s.topo
        assert t.max_depth == depth, (t.max_depth, depth)
        if unary:
            assert (t.n_children == 1).sum() >= n_leafless > 0 and t.max_children == 360
    return Shape(f"caterpillar{depth}{'u' if unary else ''}", b.done(), check)


def generated(name, n_nodes, seed=71):
    """the generator's star / deep_bushy shapes of tests/test_tree_shapes.py, topology only, generator node ids"""
    import test_tree_shapes as ts
    g = w.generate_tree(seed, n_nodes, **ts.SHAPES[name])
    sh = g.shape()
    parent = np.array(g.tree.parent, np.int32)
    g.close()

    def check(s):
        t = s.topo
        assert sh["max_children"] == t.max_children, (sh, t.max_children)
        if n_nodes == 300_000:
            assert sh["max_depth"] <= 97 and t.max_children >= 5000, sh
            assert t.max_children <= SETS_MAX_CHILDREN
        else:
            assert t.max_children > SETS_MAX_CHILDREN, sh
    return Shape(f"{name}{n_nodes}", parent, check, shuffled=False, gen_shape=sh)


# ---- rows -----------------------------------------------------------------------------------------------------------
class Rows:
    """site_ref / var_off / var_node / var_nuc of one call"""

    def __init__(self, rows):
        """rows: list of (ref mask, node ids, allele masks)"""
        self.site_ref = np.array([r[0] for r in rows], np.uint8)
        lens = [len(r[1]) for r in rows]
        self.var_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        self.var_node = np.concatenate([np.asarray(r[1], np.uint32) for r in rows] + [np.zeros(0, np.uint32)]).astype(np.uint32)
        self.var_nuc = np.concatenate([np.asarray(r[2], np.uint8) for r in rows] + [np.zeros(0, np.uint8)]).astype(np.uint8)

    @property
    def n(self):
        return len(self.site_ref)

    def row(self, r):
        a, b = int(self.var_off[r]), int(self.var_off[r + 1])
        return int(self.site_ref[r]), self.var_node[a:b], self.var_nuc[a:b]

    def args(self):
        return self.site_ref, self.var_off, self.var_node, self.var_nuc

    def has_duplicates(self):
        return any(len(np.unique(self.row(r)[1])) < len(self.row(r)[1]) for r in range(self.n))

    def has_empty_sets(self):
        return bool(((self.var_nuc & 15) == 0).any())

    def repeated(self, times):
        return Rows([self.row(r) for r in range(self.n)] * times)

    def take(self, idx):
        return Rows([self.row(int(r)) for r in idx])


def hub_edge_rows(shape):
    """Reference A.  (0) every child G, the hub observed A: the hub keeps A at cost k, every child mutates;
    (1) every child G: one mutation on the hub; (2) children alternating G / T; (3) every child G|T, the hub observed C;
    (4) every child A|G (the ambiguous set holds the reference), the hub observed C; (5) the hub's internal children
    observed, G|T and T in turn (observed internal nodes on the first and last node of the level and on both sides of
    every level-chunk edge, runs of childless nodes between them); (6) the same, reference C, with leaves next to them."""
    kids, hub_id = shape.info["kids"], shape.info["hub"]
    k = len(kids)
    alt = np.where(np.arange(k) % 2 == 0, G, T)
    ranks = shape.info["ranks"]
    inner = kids[ranks]                                    # internal children: at the level chunks' edges
    near = kids[np.setdiff1d(np.clip(np.concatenate([ranks - 3, ranks + 3]), 0, k - 1), ranks)]
    with_hub = np.concatenate([kids, [hub_id]])
    return Rows([
        (A, with_hub, np.concatenate([np.full(k, G), [A]])),
        (A, kids, np.full(k, G)),
        (A, kids, alt),
        (A, with_hub, np.concatenate([np.full(k, G | T), [C]])),
        (A, with_hub, np.concatenate([np.full(k, A | G), [C]])),
        (A, inner, np.where(np.arange(len(inner)) % 2 == 0, G | T, T)),
        (C, np.concatenate([inner, near]), np.concatenate([np.full(len(inner), G), np.full(len(near), G | C)])),
    ])


def hub_empty_rows(shape):
    """Half of the hub's children (as many as keep the sums inside `int`: empty sets cost N each) observed with an EMPTY
    allele set, every fifth of the others T, the rest G; the pairs (node, 0) then (node, G) and (node, G) then
    (node, 0) on a leaf child; every third child empty and nothing else."""
    kids = shape.info["kids"]
    k, n = len(kids), shape.topo.n
    n_empty = min(k // 2, 40000, fm.INT_LIMIT // (2 * (n + 1)))
    nuc = np.where(np.arange(k) % 5 == 1, T, G)
    nuc[np.linspace(0, k - 1, n_empty).astype(np.int64)] = 0
    leaf = int(kids[2])
    return Rows([(A, kids, nuc), (A, [leaf, leaf], [0, G]), (A, [leaf, leaf], [G, 0]),
                 (C, kids[::3][:n_empty], np.zeros(len(kids[::3][:n_empty])))])


def spine_empty_rows(shape, seed=3):
    """empty allele sets on internal (spine) nodes and on leaves of a caterpillar, next to ordinary observations"""
    rng = np.random.default_rng(seed)
    t = shape.topo
    internal = np.flatnonzero(t.n_children > 0)
    leaves = np.flatnonzero(t.n_children == 0)
    rows = []
    for _ in range(6):
        a = rng.choice(internal, min(len(internal), 7), replace=False)
        b = rng.choice(leaves, min(len(leaves), 40), replace=False)
        nodes = np.concatenate([a, b])
        nuc = (1 << rng.integers(0, 4, len(nodes)))
        nuc[rng.random(len(nodes)) < 0.3] = 0
        nuc[0] = 0
        p = rng.permutation(len(nodes))
        rows.append((1 << int(rng.integers(0, 4)), nodes[p], nuc[p]))
    return Rows(rows)


LENGTHS = (0, 1, 2, 31, 32, 33, 255, 256, 257, 5000, 50000)


def _mask(rng, p_amb):
    m = 1 << int(rng.integers(0, 4))
    if rng.random() < p_amb:
        m |= 1 << int(rng.integers(0, 4))
    return m


def shuffled_row(rng, topo, length, p_internal=0.02, p_amb=0.1, dup_share=0.05, dups=True):
    """`length` entries in shuffled order; a share of the nodes is named twice, a third of those three times, every
    entry of a node with a mask of its own (so that which entry won shows in the result)."""
    d2 = d3 = 0
    if dups and length >= 2:
        d2 = max(1, int(dup_share * length))
        d3 = min(d2 // 3 + (1 if length >= 31 else 0), length - 1 - d2) if length > 2 else 0
    uniq = length - d2 - d3
    assert 0 <= uniq <= topo.n
    internal = np.flatnonzero(topo.n_children > 0)
    leaves = np.flatnonzero(topo.n_children == 0)
    n_int = min(len(internal), int(round(p_internal * uniq))) if uniq >= 10 else int(rng.random() < p_internal)
    n_int = min(n_int, uniq)
    n_int = max(n_int, uniq - len(leaves))
    nodes = np.concatenate([rng.choice(internal, n_int, replace=False), rng.choice(leaves, uniq - n_int, replace=False)]).astype(np.int64)
    nuc = np.array([_mask(rng, p_amb) for _ in range(uniq)], np.int64)
    # entries in file order: position decides which one is "later"
    order = rng.permutation(uniq)
    nodes, nuc = list(nodes[order]), list(nuc[order])
    twice = [int(i) for i in rng.choice(uniq, d2, replace=False)] if d2 else []
    used = {nodes[i]: {nuc[i]} for i in twice}
    again = [nodes[i] for i in twice]
    for node in again + again[:d3]:
        # inserted anywhere in the row: every entry of a node has a mask of its own, whichever comes last shows
        while True:
            m = _mask(rng, 0.5)
            if m not in used[node]:
                break
        used[node].add(m)
        at = int(rng.integers(0, len(nodes) + 1))
        nodes.insert(at, node); nuc.insert(at, m)
    return np.array(nodes, np.uint32), np.array(nuc, np.uint8)


def random_rows(seed, topo, lengths=LENGTHS, per_length=2, **kw):
    rng = np.random.default_rng(seed)
    rows = []
    for L in lengths:
        if L > 0.6 * topo.n:
            continue
        for _ in range(per_length):
            nodes, nuc = shuffled_row(rng, topo, L, **kw)
            rows.append((1 << int(rng.integers(0, 4)), nodes, nuc))
    order = rng.permutation(len(rows))
    return Rows([rows[i] for i in order])


def many_rows(seed, topo, n_rows, dup_rows=0.15):
    """row lengths spread over 0 .. 600 with clusters at 127 .. 129 and 255 .. 257, shuffled entries, a share of the
    rows with duplicates of different masks"""
    rng = np.random.default_rng(seed)
    rows = []
    cluster = (127, 128, 129, 255, 256, 257)
    hi = min(600, int(0.5 * topo.n))
    for r in range(n_rows):
        L = int(cluster[r % 6]) if rng.random() < 0.3 else int(rng.integers(0, hi + 1))
        L = min(L, hi)
        nodes, nuc = shuffled_row(rng, topo, L, dups=rng.random() < dup_rows, dup_share=0.03)
        rows.append((1 << int(rng.integers(0, 4)), nodes, nuc))
    return Rows(rows)


def count_rows(seed, topo, n_sites):
    """n_sites rows: row 0 without any observation, the last row observing every node, short random rows between"""
    rng = np.random.default_rng(seed + n_sites)
    rows = [(G, [], [])]
    for r in range(1, n_sites):
        nodes, nuc = shuffled_row(rng, topo, int(rng.integers(0, 40)), dups=rng.random() < 0.2)
        rows.append((1 << int(rng.integers(0, 4)), nodes, nuc))
    everyone = rng.permutation(topo.n)
    rows[-1] = (T, everyone, (1 << rng.integers(0, 4, topo.n)))
    if n_sites == 1:
        rows = [rows[-1]]
    return Rows(rows)


# ---- expectations ---------------------------------------------------------------------------------------------------
def oracle_arrays(ot, rows, nthreads=NTHREADS):
    """oracle_mapper_body on every row (identical rows once), on at most 16 threads: the four arrays of the call"""
    L = oracle_bridge.lib()
    cache, keys = {}, []
    for r in range(rows.n):
        ref, nodes, nuc = rows.row(r)
        key = (ref, nodes.tobytes(), nuc.tobytes())
        keys.append(key)
        cache.setdefault(key, r)

    def one(r):
        ref, nodes, nuc = rows.row(r)
        vn = np.ascontiguousarray(nodes, np.int32)
        vc = np.ascontiguousarray(nuc, np.uint8)
        on = np.zeros(ot.n, np.int32); op = np.zeros(ot.n, np.uint8); om = np.zeros(ot.n, np.uint8)
        z32 = np.zeros(1, np.int32); z8 = np.zeros(1, np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        c = L.oracle_mapper_body(ot._h, ref, len(vn), p(vn if len(vn) else z32), p(vc if len(vc) else z8), p(on), p(op), p(om))
        assert c >= 0
        return on[:c].astype(np.uint32), op[:c].copy(), om[:c].copy()

    distinct = sorted(set(cache.values()))
    with ThreadPoolExecutor(max_workers=max(1, min(nthreads, 16))) as ex:
        res = dict(zip(distinct, ex.map(one, distinct)))
    per_row = [res[cache[k]] for k in keys]
    site = np.concatenate([np.full(len(x[0]), r, np.uint32) for r, x in enumerate(per_row)] + [np.zeros(0, np.uint32)])
    return (site,) + tuple(np.concatenate([x[i] for x in per_row] + [np.zeros(0, per_row[0][i].dtype)]) for i in range(3))


def assert_same(got, want, ctx):
    assert len(got[0]) == len(want[0]), f"{ctx}: {len(got[0])} mutations, expected {len(want[0])}"
    for name, a, b in zip(("site", "node", "par_nuc", "mut_nuc"), got, want):
        bad = np.flatnonzero(np.asarray(a) != np.asarray(b))
        assert bad.size == 0, (f"{ctx}: {name} differs at {bad.size} of {len(b)} mutations, first at {bad[:5].tolist()}: got "
                               f"{np.asarray(a)[bad[:5]].tolist()}, expected {np.asarray(b)[bad[:5]].tolist()} "
                               f"(rows {np.asarray(want[0])[bad[:5]].tolist()})")
