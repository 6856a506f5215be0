"""Inputs that put k_seed (wepp_amd/csrc/seed_kernels.hip) on both sides of its internal thresholds: the hit list of a
group of blocks, the hard entries and their byte counters, groups of exactly 32 blocks and their tails, the chunk
counts at which the counter rows and the slabs of 64 end, the level of 256 chunks that hands a sample to the second
pass, that pass's table of 128 samples, the routing thresholds, and ties between waves, passes and parts.

CASES[name]() returns a Case: a small tree, the environment its handle needs (WEPP_SEED_CHUNK_BLOCKS, no minimum of
hard entries or nodes; the device test turns the walks off), named samples, and which of them routing must seed.
Everything a case claims about its INPUT -- hit events per group and block, |T|, nh, H per chunk, chunks per level,
the chunk count -- is computed by tests/seed_model.py from the flat image, and the optimum by the oracle, never by the
library's placement: tests/test_seed_cases.py holds every case to its edge on the CPU, tests/test_seed_edges_gpu.py
runs them on the device.

Trees are grown by hand in DFS pre-order: the flattener visits children in ascending id order, so a node's id is its
DFS index, the first m nodes are a tree of their own, and that tree's blocks are the first blocks of the larger one
(the events in front of node m - 1 do not depend on what follows).  prefix_flat(nb) cuts a master tree at the start of
block nb: a tree of exactly nb blocks -- nb chunks with one block per chunk."""
import contextlib
import functools
import os

import numpy as np

import seed_model as sdm
import wepp_amd as w
from sweep_cases import TreeInfo
from wepp_amd import N, Reads, Tree

WIN_SIZE, WIN_STRIDE = 2560, 1024          # genome windows (device_mat.hpp): a sample inside one is no whole-genome sample
PLAN_SEED = 6
BASE_ENV = {"WEPP_SEED_MIN_HARD": "0", "WEPP_SEED_MIN_NODES": "0"}
RESERVED = 16                              # positions that are multiples of it are mutated only where a builder says so


@contextlib.contextmanager
def environment(env):
    """The variables of `env` set (None: unset) while a flat image or a handle is created."""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def ref_of(p):
    return 1 << ((p * 7 + p // 5) % 4)


def other(ref, i):
    """The i-th single allele that is not `ref`."""
    return [a for a in (1, 2, 4, 8) if a != ref][i % 3]


def grow(seed, n, genome, lo, hi, p_pop=0.45, special=None, hold=None, reserved=RESERVED, open_special=()):
    """A tree of n nodes in DFS pre-order.  Node i hangs below the node a random walk over the open path leaves on top;
    it carries lo..hi mutations at random positions that are no multiple of `reserved`, from the allele its path holds
    there to another (one in twenty ambiguous).  special[i] = the mutations of node i, which then is a child of the
    root and a leaf (open_special: those get children; special[i] = ("below", mutations): a leaf below the open special
    in front of it, which it closes); hold = (first, last): those nodes stay below node 1.  Every node draws from a
    generator of its own, so a change at node i leaves the nodes before it as they were."""
    special = special or {}
    parent, muts, stack, geno = [-1], [[]], [0], [{}]
    for i in range(1, n):
        rng = np.random.default_rng([seed, i])
        below = i in special and len(special[i]) == 2 and special[i][0] == "below"
        if below:
            ml = list(special[i][1])
        elif i in special:
            del stack[1:], geno[1:]
            ml = list(special[i])
        else:
            floor = 2 if hold and hold[0] <= i <= hold[1] else 1
            while len(stack) > floor and rng.random() < p_pop:
                stack.pop()
                geno.pop()
            ml = []
            for p in sorted(set(int(x) for x in rng.integers(1, genome + 1, size=int(rng.integers(lo, hi + 1))))):
                if p % reserved == 0:
                    continue
                cur = geno[-1].get(p, ref_of(p))
                m = cur
                while m == cur:
                    m = 1 << int(rng.integers(0, 4))
                    if rng.random() < 0.05:
                        m |= 1 << int(rng.integers(0, 4))
                ml.append((p, ref_of(p), cur, m))
        g = dict(geno[-1])
        for (p, _, _, m) in ml:
            g[p] = m
        parent.append(stack[-1])
        muts.append(ml)
        if below:
            del stack[1:], geno[1:]
        elif i not in special or i in open_special:
            stack.append(i)
            geno.append(g)
    return Tree.from_lists(parent, muts)


class Flat:
    """A tree flattened with `stride` blocks per chunk: TreeInfo (tests/sweep_cases.py) and the seed model."""

    def __init__(self, tree, stride):
        with environment({"WEPP_SEED_CHUNK_BLOCKS": str(stride)}):
            self.info = TreeInfo(tree)
        self.tree, self.stride = tree, stride
        self.model = sdm.SeedModel(self.info.flat)
        assert self.model.built and self.model.stride == stride
        t = tree
        self.allele = {}                                # position -> the allele of its first mutation in the tree
        for p, m in zip(t.mut_pos.tolist(), t.mut_mut.tolist()):
            self.allele.setdefault(p, m)


def in_one_window(S):
    """k_route's test: all listed positions inside the genome window of the first one."""
    return not S or S[-1][0] < S[0][0] // WIN_STRIDE * WIN_STRIDE + WIN_SIZE


def spanning(S, far):
    """S, with a missing entry at `far` (beyond the tree) when it would fit one genome window."""
    S = sorted(S)
    return S + [(far, ref_of(far), N, 1)] if in_one_window(S) else S


class Case:
    """name; key of the tree (cases with the same key and environment share a device handle); tree; blocks per chunk;
    samples {name: entries}; seeded = the names routing must send to the seed plan (default: all); min_hard: the
    handle's WEPP_SEED_MIN_HARD (None: the product's default); counts: the prefixes of the batch to place; deferral:
    the case hands samples to the second pass (the device test adds its runs); facts: what the builder aimed at."""

    def __init__(self, name, key, flat, samples, seeded=None, min_hard="0", counts=None, deferral=False, facts=None):
        self.name, self.key, self.flat, self.tree, self.stride = name, key, flat, flat.tree, flat.stride
        self.samples = dict(samples)
        self.names = list(self.samples)
        self.seeded = set(self.names if seeded is None else seeded)
        self.env = dict(BASE_ENV, WEPP_SEED_CHUNK_BLOCKS=str(flat.stride), WEPP_SEED_MIN_HARD=min_hard)
        self.counts = counts or (len(self.names),)
        self.deferral = deferral
        self.facts = facts or {}
        self.model = flat.model

    def lists(self):
        return [self.samples[n] for n in self.names]

    @property
    def reads(self):
        return Reads.from_lists(self.lists())

    def over_max_hard(self):
        return any(len(self.model.hard_entries(S)[0]) > sdm.SEED_MAX_HARD for S in self.lists())


CASES = {}


def case(fn):
    CASES[fn.__name__] = functools.lru_cache(maxsize=None)(fn)
    return CASES[fn.__name__]


# ---- picking positions by the hit events they give -------------------------------------------------------------------
def hit_sample(flat, c, group, target, seed, both_rounds=False, far=None):
    """A sample with exactly `target` hit events in group `group` of chunk c: positions of the group's events taken in
    event order (both_rounds: alternately from the first and the last round of 512 slots) while their events in the
    group fit.  Seven in ten entries carry the tree's allele, the others the reference allele or N."""
    m = flat.model
    b0, b1 = m.chunk_blocks(c)
    bg = b0 + group * sdm.GROUP_BLOCKS
    ng = min(sdm.GROUP_BLOCKS, b1 - bg)
    e0, e1 = int(m.blk_eoff[bg]), int(m.blk_eoff[bg + ng])
    ev = m.ev_pos[e0:e1]
    n_at = {}
    for p in ev.tolist():
        if p != sdm.W_PAD_POS:
            n_at[p] = n_at.get(p, 0) + 1
    order = [int(p) for p in ev.tolist() if p != sdm.W_PAD_POS]
    if both_rounds:
        head = order[:sdm.SCAN_ROUND // 2]
        tail = [int(p) for p in ev[(len(ev) - 1) // sdm.SCAN_ROUND * sdm.SCAN_ROUND:].tolist() if p != sdm.W_PAD_POS]
        order = [p for pair in zip(head, tail) for p in pair] + order
    else:
        order = order[::max(1, len(order) // target)] + order          # spread over the group's blocks
    chosen, total = [], 0
    for p in order:
        if p not in chosen and total + n_at[p] <= target:
            chosen.append(p)
            total += n_at[p]
    assert total == target, (total, target)
    rng = np.random.default_rng(seed)
    S = []
    for p in chosen:
        u = rng.random()
        S.append((p, ref_of(p), flat.allele[p], 0) if u < 0.7 else (p, ref_of(p), ref_of(p), 0) if u < 0.85 else (p, ref_of(p), N, 1))
    return spanning(S, (far or m.max_pos) + 3000)


# ---- the hit list: one block per chunk, a group is one block --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hits_flat():
    """600 nodes of 1..3 mutations, hardly a position mutated twice: blocks close at 128 events."""
    return Flat(grow(11, 600, 12000, 1, 3), 1)


def fullest_block(flat):
    m = flat.model
    real = [int((m.ev_pos[m.blk_eoff[b]:m.blk_eoff[b + 1]] != sdm.W_PAD_POS).sum()) for b in range(m.nb)]
    return int(np.argmax(real)), max(real)


@case
def hits_one_block():
    """63, 64, 65, 96 and 97 hit events, and every event of the block, in ONE block (one block per chunk): apply_hits with a
    full round of 64, a second round, the last list that fits and the first that does not."""
    flat = hits_flat()
    b, real = fullest_block(flat)
    targets = dict(h63=63, h64=64, h65=65, h96=96, h97=97, hall=real)
    samples = {n: hit_sample(flat, b, 0, h, 100 + h) for n, h in targets.items()}
    return Case("hits_one_block", "hits", flat, samples, facts=dict(chunk=b, targets=targets))


# ---- groups of 32 blocks, tails, rounds of 512 events: strides 32, 33 and 40 -----------------------------------------
@functools.lru_cache(maxsize=None)
def groups_tree():
    return grow(12, 2600, 20000, 1, 3)


def _groups_case(stride):
    flat = Flat(groups_tree(), stride)
    m = flat.model
    samples, targets = {}, {}
    # (chunk, group) to aim at: the first group of 32 blocks, the tail group of chunk 0, the last chunk of the tree
    aims = {"first": (0, 0), "last_chunk": (m.nch - 1, 0)}
    if stride > sdm.GROUP_BLOCKS:
        aims["tail"] = (0, 1)
    for tag, (c, g) in aims.items():
        for h in (96, 97):
            samples["%s_%d" % (tag, h)] = hit_sample(flat, c, g, h, 1000 * stride + h + 7 * c + g)
            targets["%s_%d" % (tag, h)] = (c, g, h)
    # more than 512 events in the group, hits in the first and in the last round, the list not overflowing / overflowing
    for h in (80, 140):
        samples["rounds_%d" % h] = hit_sample(flat, 0, 0, h, 2000 * stride + h, both_rounds=True)
        targets["rounds_%d" % h] = (0, 0, h)
    return Case("groups_%d" % stride, "groups", flat, samples, facts=dict(targets=targets))


for _s in (32, 33, 40):
    def _gc(stride=_s):
        return _groups_case(stride)
    _gc.__name__ = "groups_%d" % _s
    _gc.__doc__ = ("%d blocks per chunk: groups of exactly 32 blocks%s, a short last chunk; 96 and 97 hit events spread over the "
                   "blocks of a group; more than 512 events in a group with hits in both rounds." % (_s, ", a tail group of %d" % (_s - 32) if _s > 32 else ""))
    case(_gc)


# ---- hard entries -----------------------------------------------------------------------------------------------------
HARD_X = 300                 # mutations of node X
HARD_GENOME = 3200


@functools.lru_cache(maxsize=None)
def hard_flat():
    """Root -> X, a node with 300 mutations at the positions 8, 16, ... (a one-node block of 300 events) above 150
    nodes; 150 more nodes beside X; a last leaf that mutates position 3200, the tree's largest."""
    xm = [(8 * i, ref_of(8 * i), ref_of(8 * i), other(ref_of(8 * i), i)) for i in range(1, HARD_X + 1)]
    last = [(HARD_GENOME, ref_of(HARD_GENOME), ref_of(HARD_GENOME), other(ref_of(HARD_GENOME), 1))]
    side = [(3, ref_of(3), ref_of(3), other(ref_of(3), 0))]
    # (no other node mutates a multiple of 8: X's positions are X's alone)
    return Flat(grow(13, 303, HARD_GENOME - 1, 1, 3, special={1: xm, 152: side, 302: last}, hold=(2, 151), reserved=8, open_special=(1,)), 1)


def x_entries(h):
    return [(8 * i, ref_of(8 * i), other(ref_of(8 * i), i), 0) for i in range(1, h + 1)]


HARD_COUNTS = (14, 15, 16, 30, 31, 254, 255, 256, 300)


@case
def hard_entries():
    """14 .. 255 hard entries that one chunk's signature serves all (X's own mutations): the SWAR flush at 15, the byte
    counter at 255, SEED_MAX_HARD; hard entries at max_pos and beyond it; no hard entry inside the tree; none at all."""
    flat = hard_flat()
    m = flat.model
    mp = m.max_pos
    fill = [(2801, ref_of(2801), ref_of(2801), 0), (3001, ref_of(3001), N, 1)]
    samples = {"hard_%d" % h: sorted(x_entries(h) + fill) for h in HARD_COUNTS if h <= sdm.SEED_MAX_HARD}
    beyond = [(mp + 1, 1, 2, 0), (mp + 90, 2, 4, 0), (mp + 5000, 4, 8, 0)]
    samples["hard_255_beyond"] = sorted(x_entries(255) + fill + beyond)
    samples["at_max_pos"] = sorted(x_entries(3) + [(mp, ref_of(mp), flat.allele[mp], 0)] + beyond[:2])
    samples["all_beyond"] = sorted([(8, ref_of(8), ref_of(8), 0), (500, ref_of(500), N, 1)] + beyond)
    samples["no_hard"] = sorted([(8, ref_of(8), ref_of(8) | other(ref_of(8), 1), 0), (500, ref_of(500), N, 1), (2801, ref_of(2801), ref_of(2801), 0), (mp + 7, 1, N, 1)])
    # the exact genotype of a node beside X, plus three hard entries beyond the tree: the optimum, 3, is found at the top
    # level.  The node is the first of its chunk and its parent sits in the chunk before: that chunk serves all but the
    # node's own one to three mutations.
    node = next(d for d in (int(x) for x in m.chunk_lo[1:-1]) if d > 153 and m.chunk_of_dfs(int(flat.tree.parent[d])) == m.chunk_of_dfs(d) - 1
                and len(flat.info.genotype(d)) >= 5)
    samples["node_beyond"] = sorted(flat.info.genotype(node) + beyond)
    return Case("hard_entries", "hard", flat, samples, facts=dict(node=node, beyond=len(beyond)))


@case
def hard_over():
    """256 and 300 hard entries inside the tree: the kernel counts 255 of them, whichever its atomics leave."""
    flat = hard_flat()
    mp = flat.model.max_pos
    fill = [(2801, ref_of(2801), ref_of(2801), 0), (3001, ref_of(3001), N, 1)]
    samples = {"hard_%d" % h: sorted(x_entries(h) + fill) for h in HARD_COUNTS if h > sdm.SEED_MAX_HARD}
    samples["hard_300_beyond"] = sorted(x_entries(300) + fill + [(mp + 1, 1, 2, 0)])
    samples["hard_20"] = sorted(x_entries(20) + fill)
    return Case("hard_over", "hard", flat, samples)


# ---- chunk counts, levels, the second pass: prefixes of one master tree, one block per chunk -------------------------
Q1, Q2 = 16, 32              # the twins' shared positions
TWIN_EVERY = 32              # a twin every 32 nodes, kinds A and B in turn
MASTER_NODES, MASTER_GENOME = 12000, 8000


def twin_b():
    """Twin B, a leaf child of the root: only an allele at Q2."""
    return [(Q2, ref_of(Q2), ref_of(Q2), other(ref_of(Q2), 0))]


def twin_a(i):
    """Twin A, a leaf with the allele the tie sample lists at Q1, below a child of the root with one mutation of its
    own (U_i), which the sample does not list: the leaf costs the sample that one mutation."""
    u = RESERVED * (3 + (i // TWIN_EVERY) % 490)
    return [(u, ref_of(u), ref_of(u), other(ref_of(u), i))], ("below", [(Q1, ref_of(Q1), ref_of(Q1), other(ref_of(Q1), 0))])


def master(n=MASTER_NODES, extra=()):
    """The first n of 12 000 nodes of 2..6 mutations (about 18 nodes per block).  Every 32 nodes the walk returns to the
    root with a TWIN: kind A (two nodes) and kind B in turn, the first one at node 96 (chunk 0 holds none).  extra:
    nodes at which a twin of kind B and one of kind A follow each other."""
    special, opened = {}, []
    for i in range(3 * TWIN_EVERY, n - 1, TWIN_EVERY):
        if (i // TWIN_EVERY) % 2:
            special[i], special[i + 1] = twin_a(i)
            opened.append(i)
        else:
            special[i] = twin_b()
    for i in extra:
        special[i] = twin_b()
        special[i + 1], special[i + 2] = twin_a(i + 1)
        opened.append(i + 1)
    return grow(14, n, MASTER_GENOME, 2, 6, special=special, open_special=tuple(j for j in opened if special[j + 1][0] == "below"))


def blocks_of(tree):
    with environment({"WEPP_SEED_CHUNK_BLOCKS": "1"}):
        return w.FlatView(tree).get("blk_node0").astype(np.int64)


@functools.lru_cache(maxsize=None)
def master_blocks():
    return blocks_of(master())


def cut(t, n):
    e = int(t.mut_off[n])
    return Tree(t.parent[:n], t.mut_off[:n + 1], t.mut_pos[:e], t.mut_ref[:e], t.mut_mut[:e], t.mut_par[:e])


@functools.lru_cache(maxsize=None)
def prefix_flat(nb, twin_in_last=False):
    """The master tree cut at the start of block nb: exactly nb blocks, nb chunks.  twin_in_last: the nodes behind
    the first one of the last block are a twin of kind B and one of kind A (the nodes before them, and so the blocks
    before the last, stay as they were)."""
    if not twin_in_last:
        return Flat(cut(master(), int(master_blocks()[nb])), 1)
    first = int(master_blocks()[nb - 1])
    t = master(min(MASTER_NODES, first + 200), (first + 1,))       # (a block holds 64 nodes at most)
    return Flat(cut(t, int(blocks_of(t)[nb])), 1)


def tie_a(far):
    """One hard entry, the twins' allele at Q1: the root (Q1 unserved) and every twin A (its parent's mutation) score 1."""
    return [(Q1, ref_of(Q1), other(ref_of(Q1), 0), 0), (Q1 + 1000, ref_of(Q1 + 1000), N, 1), (far, ref_of(far), N, 1)]


def tie_b(far, i=0):
    """No hard entry: at Q2 the reference allele or the twins'.  The root and every twin B score 0.  i varies the
    missing entries (the answer does not depend on them)."""
    amb = ref_of(Q2) | other(ref_of(Q2), 0)
    return [(Q2, ref_of(Q2), amb, 0), (Q2 + 1001 + i, ref_of(Q2 + 1001 + i), N, 1), (far + i, ref_of(far + i), N, 1)]


def node_samples(flat, chunks, seed):
    """The genotype of the last node of each of `chunks` (its words at most 200), made to span two genome windows."""
    out = {}
    for c in chunks:
        d = int(flat.model.chunk_lo[c + 1]) - 1
        g = flat.info.genotype(d)[:200]
        out["node_in_chunk_%d" % c] = spanning(g, flat.model.max_pos + 3000 + seed)
    return out


NCH = (7, 8, 9, 63, 64, 65, 511, 512, 513)


def _nch_case(nch):
    flat = prefix_flat(nch, twin_in_last=True)
    far = flat.model.max_pos + 4000
    samples = dict(tie_a=tie_a(far), tie_b=tie_b(far))
    samples.update(node_samples(flat, sorted({0, nch // 2, nch - 2, nch - 1}), nch))
    return Case("nch_%d" % nch, "prefix_%d_twin" % nch, flat, samples, deferral=nch >= sdm.SEED_HEAVY_LEVEL_MIN, facts=dict(nch=nch))


for _n in NCH:
    def _nc(nch=_n):
        return _nch_case(nch)
    _nc.__name__ = "nch_%d" % _n
    _nc.__doc__ = ("A tree of exactly %d chunks, a twin in the last one: the counter words, the guard of the last word, the "
                   "last slab; ties between chunks of different slabs%s." % (_n, " and, handed over at the top level, of different parts" if _n > 512 else ""))
    case(_nc)


@case
def defer_255():
    """255 chunks, a sample without hard entries: one level of 255 chunks, which stays in the first pass."""
    flat = prefix_flat(255)
    far = flat.model.max_pos + 4000
    return Case("defer_255", "prefix_255", flat, dict(tie_b=tie_b(far), tie_a=tie_a(far)), facts=dict(nch=255))


@case
def defer_256():
    """256 chunks: the same sample's only level holds 256 chunks -- handed over at the TOP level, the first pass
    evaluates nothing.  A sample with one hard entry leaves 255 chunks or fewer on either level and stays."""
    flat = prefix_flat(256)
    far = flat.model.max_pos + 4000
    return Case("defer_256", "prefix_256", flat, dict(tie_b=tie_b(far), tie_a=tie_a(far)), deferral=True, facts=dict(nch=256))


@case
def defer_lower():
    """400 chunks, one hard entry: the twins' chunks (level 1) are evaluated by the first pass, which finds the score 1;
    level 0 holds 256 chunks or more and goes to the second pass, where the root ties with it."""
    flat = prefix_flat(400)
    far = flat.model.max_pos + 4000
    return Case("defer_lower", "prefix_400", flat, dict(tie_a=tie_a(far), tie_b=tie_b(far)), deferral=True, facts=dict(nch=400))


@case
def heavy_cap():
    """129 samples that are all handed over on the 256-chunk tree, placed as batches of 128 (the table is full) and
    of 129 (one sample stays with its own workgroup)."""
    flat = prefix_flat(256)
    far = flat.model.max_pos + 4000
    samples = {"tie_b_%d" % i: tie_b(far, i) for i in range(sdm.SEED_HEAVY_CAP + 1)}
    return Case("heavy_cap", "prefix_256", flat, samples, counts=(sdm.SEED_HEAVY_CAP, sdm.SEED_HEAVY_CAP + 1), deferral=True)


# ---- routing ----------------------------------------------------------------------------------------------------------
def long_sample(flat, k, seed):
    """k entries: every mutated position of the tree, then positions beyond it; tree alleles, reference alleles, N."""
    m = flat.model
    rng = np.random.default_rng(seed)
    pos = sorted(p for p in flat.allele if p > 0)
    pos = pos[::max(1, len(pos) // k)][:k]
    pos += list(range(m.max_pos + 2, m.max_pos + 2 + 3 * (k - len(pos)), 3))
    S = []
    for p in pos:
        u = rng.random()
        a = flat.allele.get(p, other(ref_of(p), p))
        S.append((p, ref_of(p), a, 0) if u < 0.5 else (p, ref_of(p), ref_of(p), 0) if u < 0.8 else (p, ref_of(p), N, 1))
    assert len(S) == k
    return S


@case
def route_entries():
    """SEED_MAX_ENTRIES: a sample of 4096 entries is seeded, one of 4097 swept; a sample of ONE entry (beyond every
    genome window of the tree) beside them: the words' room in LDS is the batch maximum, 4096."""
    flat = hits_flat()
    far = flat.model.max_pos + 100000
    samples = dict(one=[(far, ref_of(far), other(ref_of(far), 0), 0)], k4096=long_sample(flat, sdm.SEED_MAX_ENTRIES, 1),
                   k4097=long_sample(flat, sdm.SEED_MAX_ENTRIES + 1, 2), k100=long_sample(flat, 100, 3))
    return Case("route_entries", "hits", flat, samples, seeded=("one", "k4096", "k100"))


@case
def route_min_hard():
    """The product's minimum of hard entries, 3: samples with 2 and with 3 of them (and as many other entries)."""
    flat = hits_flat()
    ps = sorted(p for p in flat.allele if p > 0 and (flat.allele[p] & ref_of(p)) == 0)
    lo, hi = ps[:6], [p for p in ps if p >= ps[0] // WIN_STRIDE * WIN_STRIDE + WIN_SIZE][:6]

    def sample(n_hard):
        S = []
        for i, p in enumerate(lo[:3] + hi[:3]):
            a = flat.allele[p]
            hard = i < n_hard and (a & ref_of(p)) == 0
            S.append((p, ref_of(p), a if hard else ref_of(p), 0))
        return sorted(S)
    samples = dict(hard_2=sample(2), hard_3=sample(3), hard_4=sample(4))
    return Case("route_min_hard", "hits", flat, samples, seeded=("hard_3", "hard_4"), min_hard=None)


# ---- what the oracle and the model say about a case ------------------------------------------------------------------
_EXPECT = {}


def expectations(case, oracle):
    """Per sample: the oracle's optimum (best), the root's score, the chunks that hold an optimal node, num_best; the
    model's must / may, and `settled`: an optimal node sits in a chunk of the top level, so exactly the must chunks
    are evaluated (seed_model.settled_at_the_top)."""
    if case.name not in _EXPECT:
        ot = oracle.OracleTree(case.tree)
        m, out = case.model, {}
        for n in case.names:
            S = case.samples[n]
            o = ot.place_sample(*(list(zip(*S)) if S else ([], [], [], [])), per_node_scores=True, want_best_vec=True)
            best, root = int(o["score"]), int(o["node_scores"][0])
            must, may = m.must_may(S, best, root)
            vec = [int(j) for j in o["best_j_vec"]]
            out[n] = dict(best=best, root=root, must=must, may=may, num_best=int(o["num_best"]),
                          chunks=sorted(set(m.chunk_of_bfs(j) for j in vec)), settled=m.settled_at_the_top(S, best, vec))
        ot.close()
        _EXPECT[case.name] = out
    return _EXPECT[case.name]


def evaluated_bounds(case, oracle, count=None):
    """(lo, hi) of the chunks the device may report as evaluated for the first `count` samples that routing seeds."""
    ex = expectations(case, oracle)
    names = [n for n in case.names[:count] if n in case.seeded]
    lo = sum(ex[n]["must"] for n in names)
    hi = sum(ex[n]["must"] if ex[n]["settled"] else ex[n]["may"] for n in names)
    return lo, hi
