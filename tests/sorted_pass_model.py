"""Sequential model of the sorted pass of a read with more than 64 events (wepp_amd/csrc/place_dev.hpp: sorted_build,
sorted_query) beside the all-pairs definition it replaces (walk_model.py: place_all_pairs, the inner loop restated
here field by field).  An entry is (node, end, pk): a mutation of stream node `node` whose subtree ends in front of
`end`, and the packed adjustments of pack_adjust -- the delta biased by PK_BIAS in the low byte, a one in the top byte.
Both functions return one (cb, cB, T, stopA, stopB, fl) per entry.  NOT a product path."""
from bisect import bisect_left

import numpy as np

from sweep_model import enter_delta, own_adjust

M = 0xFFFFFFFF
NONE = 0xFFFFFFFF
PK_BIAS = 2
MAX_EVENTS = 256
FIELDS = ("cb", "cB", "T", "stopA", "stopB", "fl")


def pack(d, adj, dcom):
    assert -2 <= d <= 2 and -1 <= adj <= 1 and -1 <= dcom <= 1
    return (d + PK_BIAS) | (adj + PK_BIAS) << 8 | (dcom + PK_BIAS) << 16 | 1 << 24


def entries_of(model, S):
    """The entries of read S in walk_model.WalkModel `model`'s stream, in the order of the concatenated lists."""
    npos = len(model.ix_off) - 1
    ents = []
    for j, (p, _, _, _) in enumerate(S):
        if p >= npos:
            continue
        for q in range(int(model.ix_off[p]), int(model.ix_off[p + 1]) - 1):
            node, end, w = int(model.ix_node[q]), int(model.ix_end[q]), int(model.ix_word[q])
            d = enter_delta(w, S[j]) if (end > node + 1 or node == 0) else 0
            a1, a2 = own_adjust(w, S[j])
            ents.append((node, end, pack(d, a1, a2)))
    return ents


def all_pairs(ents):
    """The definition: every entry against every entry, with the kernel's wrapping differences."""
    out = []
    for mg, (n, e, _) in enumerate(ents):
        cb = cB = T = fl = 0
        stopA = stopB = M
        sA = n + 1
        for g, (nl, el, pl) in enumerate(ents):
            dl = (pl & 0xFF) - PK_BIAS
            nl1, span = nl + 1, (el - nl - 1) & M
            if dl != 0:
                if ((n - nl1) & M) < span:
                    cb += dl
                if ((e - nl1) & M) < span:
                    cB += dl
            if nl == n:
                T = (T + pl) & M
                fl |= 1 if g < mg else 0
            if el == e and g < mg:
                fl |= 2
            stopA = min(stopA, (nl - sA) & M, (el - sA) & M)
            stopB = min(stopB, (2 * nl - 2 * e) & M, (2 * el - 1 - 2 * e) & M)
        out.append((cb, cB, T, stopA, stopB, fl))
    return out


def sorted_pass(ents, N=MAX_EVENTS):
    """The sorted formulation, as the kernel lays it out: N slots, padding keys NONE behind every real key, the entry
    index in the low byte of a key, inclusive prefix sums of the biased deltas and of the (wrapping) packed words."""
    E = len(ents)
    assert E <= N <= MAX_EVENTS
    node = [ents[i][0] if i < E else NONE for i in range(N)]
    end = [ents[i][1] if i < E else NONE for i in range(N)]
    pk = [ents[i][2] if i < E else 0 for i in range(N)]
    ka = sorted(node[i] << 8 | i for i in range(N))
    kb = sorted(end[i] << 8 | i for i in range(N))
    ppk, dla, dlb = [], [], []
    sp = sa = sb = 0
    for p in range(N):
        va = pk[ka[p] & 0xFF] if ka[p] >> 8 != NONE else 0
        vb = pk[kb[p] & 0xFF] & 0xFF if kb[p] >> 8 != NONE else 0
        sp, sa, sb = (sp + va) & M, sa + (va & 0xFF), sb + vb
        ppk.append(sp); dla.append(sa); dlb.append(sb)
    assert sa < 1 << 16 and sb < 1 << 16            # (the kernel keeps both in the halves of one word)
    d_node = lambda c: dla[c - 1] - PK_BIAS * c if c else 0
    d_end = lambda c: dlb[c - 1] - PK_BIAS * c if c else 0
    at = lambda k, c: k[c] >> 8 if c < N else NONE
    out = []
    for i, (n, e, _) in enumerate(ents):
        r0, r1, r2 = bisect_left(ka, n << 8), bisect_left(ka, (n + 1) << 8), bisect_left(kb, (n + 1) << 8)
        r3, r4, r5 = bisect_left(ka, e << 8), bisect_left(kb, (e + 1) << 8), bisect_left(kb, e << 8)
        cb, cB = d_node(r0) - d_end(r2), d_node(r3) - d_end(r4)
        T = ((ppk[r1 - 1] if r1 else 0) - (ppk[r0 - 1] if r0 else 0)) & M
        fl = (1 if ka[r0] & 0xFF != i else 0) | (2 if kb[r5] & 0xFF != i else 0)
        stopA = (min(at(ka, r1), at(kb, r2)) - (n + 1)) & M
        na, eb = at(ka, r3), at(kb, r4)
        stopB = min(((na - e) << 1) & M if na != NONE else NONE, (((eb - e) << 1) - 1) & M if eb != NONE else NONE)
        out.append((cb, cB, T, stopA, stopB, fl))
    return out


def canonical(acc):
    """stopB without a cut behind the end: the all-pairs minimum is then some wrapped difference >= 0x80000000, the sorted
    pass says NONE, and `finish` reads every such value as "to the end of the stream"."""
    cb, cB, T, stopA, stopB, fl = acc
    return (cb, cB, T, stopA, NONE if stopB >= 0x80000000 else stopB, fl)


def assert_same(got, want, ctx=""):
    assert len(got) == len(want), (ctx, len(got), len(want))
    for i, (g, x) in enumerate(zip(got, want)):
        g, x = canonical(tuple(int(v) for v in g)), canonical(x)
        for name, a, b in zip(FIELDS, g, x):
            assert a == b, f"{ctx}: entry {i} of {len(want)}: {name} is {a}, all pairs give {b}"


# ---- hand-made lists ------------------------------------------------------------------------------------------------
def rand_pk(rng):
    return pack(int(rng.integers(-2, 3)), int(rng.integers(-1, 2)), int(rng.integers(-1, 2)))


def random_tree_entries(rng, E, n_nodes, leaves_only=False):
    """E entries on the nodes of a random tree of n_nodes in preorder (parent of v: a node in front of it), nodes drawn
    with repetition, so that several entries share a node, subtree ends coincide and nodes sit at other entries' ends."""
    # a valid preorder: the parent of v is v - 1 or one of its ancestors -- walk its chain up by a random number of steps
    par = [-1] * n_nodes
    for v in range(1, n_nodes):
        p = v - 1
        for _ in range(int(rng.integers(0, 4))):
            if par[p] < 0:
                break
            p = par[p]
        par[v] = p
    end = [v + 1 for v in range(n_nodes)]
    for v in range(n_nodes - 1, 0, -1):
        end[par[v]] = max(end[par[v]], end[v])
    nodes = [v for v in range(n_nodes) if end[v] == v + 1] if leaves_only else list(range(n_nodes))
    pick = rng.choice(nodes, size=E, replace=True)
    return [(int(v), int(end[v]), rand_pk(rng)) for v in pick]


EDGE_SIZES = (1, 64, 65, 128, 129, 192, 193, 255, 256)


def hand_made(rng):
    """(name, entries) of the shapes the sort must get right."""
    cases = []
    for E in EDGE_SIZES:
        cases.append((f"random tree, E={E}", random_tree_entries(rng, E, max(2, E // 2))))
        cases.append((f"one node, E={E}", [(5, 9, rand_pk(rng)) for _ in range(E)]))
        cases.append((f"all ends equal, E={E}", [(int(v), 400, rand_pk(rng)) for v in rng.integers(0, 400, E)]))
        # a chain in which every node sits at the end of the entry before it: (0,3) (3,6) (6,9) ..., shuffled, with repeats
        chain = [(3 * int(v), 3 * int(v) + 3, rand_pk(rng)) for v in rng.integers(0, max(1, E // 3), E)]
        cases.append((f"node == end chains, E={E}", chain))
        cases.append((f"leaves only, E={E}", random_tree_entries(rng, E, max(2, 3 * E), leaves_only=True)))
        root = random_tree_entries(rng, E, max(2, E))
        root[int(rng.integers(0, E))] = (0, max(2, E), rand_pk(rng))
        cases.append((f"the root entry, E={E}", root))
        top = (1 << 25) - 1
        big = [(top - 1 - int(v), top, rand_pk(rng)) for v in rng.integers(0, 40, E)]
        big[0] = (0, top, rand_pk(rng))
        cases.append((f"keys at 2^25 - 1, E={E}", big))
    return cases
