"""Builders and a small model for the edges of wepp_epp_map (tests/test_epp_cases.py holds every builder to the edge
it is for, on the CPU, against the oracle and this model alone; tests/test_epp_map_edges_gpu.py runs them on the GPU).

The model restates, in plain Python/NumPy, the three things of the library that decide which branch of the sweep runs:

  plan()    the host plan of epp_sweep_pass1 (epp_sweep.cpp): reads by (start, end, index), tiles of 64 * rpl reads,
            groups of tiles_per_group tiles, the window of every tile and group;
  stream()  the MAT's EPP event stream as flatmat.hpp defines it;
  chunks()  the cuts of a window stream, 1024 events apart under the default WEPP_EPP_TARGET_JOBS.

Nothing here looks at what the library returns."""
from fractions import Fraction

import numpy as np

import epp_fuzz
import fuzz_trees as ft
from wepp_amd import EppReads, Tree

LANES = 64                 # reads per lane slot of a tile (a tile is 64 * rpl reads)
MAX_GROUPS = 512           # EPP_MAX_GROUPS, epp.hpp
CHUNK_EVENTS = 1024        # the floor of chunk_events, epp_sweep.cpp
SEL_EVENTS = 1024          # EPP_SEL_EVENTS, epp.hpp: events of the MAT's stream per selection block
SEL_SCAN_WIDTH = 256       # blocks k_epp_select_scan takes per round: beyond it the carry runs
TARGET_JOBS = 262144       # EPP_TARGET_JOBS, epp_sweep.cpp
LDS_LIMIT = 150 * 1024     # epp_sweep_pass1: "reads too long" above it
RPL4_TABLE_LIMIT = 48 * 1024
ORACLE_LIST_CAP = 2048     # MAX_CACHED_EPP_SIZE, oracle/epp_oracle.c


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def effective_rpl(start, end, rpl):
    """WEPP_EPP_RPL=4 holds only while the allele table of 256 reads stays within 48 KiB (epp_sweep_pass1)."""
    longest = int((np.asarray(end, np.int64) - np.asarray(start, np.int64)).max())
    if rpl == 4 and ((longest >> 3) + 1) * 64 * 4 * 4 > RPL4_TABLE_LIMIT:
        return 1
    return rpl


def lds_bytes(span, rpl=1):
    """LDS the plan asks for with one tile window and one longest read of `span` = end - start."""
    return 4 * ((span >> 5) + 1 + 64 * rpl * ((span >> 3) + 1))


def plan(start, end, rpl):
    """Host plan of epp_sweep_pass1 for reads with windows [start, end] at `rpl` reads per lane (the value in force:
    see effective_rpl).  Windows are inclusive [min start, max end]."""
    start = np.asarray(start, np.int64)
    end = np.asarray(end, np.int64)
    R = len(start)
    order = np.lexsort((np.arange(R), end, start))
    ts = LANES * rpl
    ntiles = -(-R // ts)
    tpg = max(1, -(-ntiles // MAX_GROUPS))
    G = -(-ntiles // tpg)
    s, e = start[order], end[order]
    t0 = np.arange(0, R, ts)
    tile_ws, tile_we = np.minimum.reduceat(s, t0), np.maximum.reduceat(e, t0)
    g0 = np.arange(0, ntiles, tpg)
    return dict(order=order, rpl=rpl, tile_reads=ts, ntiles=ntiles, tpg=tpg, G=G, tile_ws=tile_ws, tile_we=tile_we,
                tile_group=np.arange(ntiles) // tpg, group_tile0=g0,
                group_ntiles=np.minimum(tpg, ntiles - g0),
                group_ws=np.minimum.reduceat(tile_ws, g0), group_we=np.maximum.reduceat(tile_we, g0))


def preorder(tree):
    """Pre-order index -> caller id and the last pre-order index of every subtree.  Children are visited in ascending
    id order: flatmat.cpp fills the children CSR by ascending id ("children CSR (ascending id order)") and its DFS pushes
    them on the stack in reverse, so the smallest id is popped first."""
    n = tree.n_nodes
    kids = [[] for _ in range(n)]
    root = -1
    for i in range(n):
        p = int(tree.parent[i])
        if p < 0:
            root = i
        else:
            kids[p].append(i)
    dfs2id, stack = [], [root]
    while stack:
        c = stack.pop()
        dfs2id.append(c)
        stack.extend(reversed(kids[c]))
    dfs2id = np.array(dfs2id, np.int64)
    dfs_of = np.empty(n, np.int64)
    dfs_of[dfs2id] = np.arange(n)
    dfs_end = np.arange(n)
    for d in range(n - 1, 0, -1):
        pd = dfs_of[tree.parent[dfs2id[d]]]
        dfs_end[pd] = max(dfs_end[pd], dfs_end[d])
    return dfs2id, dfs_end


def stream(tree):
    """The EPP event stream (flatmat.hpp, "EPP event stream"; built at the end of flatten_tree in flatmat.cpp): a
    pre-order walk, every non-masked mutation once as an enter event at its node, in the node's own (position) order,
    and once as an exit event when the subtree is done.  Exit order as flatmat.cpp's `close` has it: before node d is
    entered, every open node whose subtree ended before d is closed innermost first, each node's mutations again in
    their own order; whatever is still open after the last node is closed the same way.
    Returns pos, node (nodes entered before the event: the node's index for an enter, one past the subtree's last
    index for an exit), exit (bool) and owner (pre-order index of the node that carries the mutation)."""
    dfs2id, dfs_end = preorder(tree)
    pos, node, ext, owner = [], [], [], []
    open_ = []

    def close(a):
        i = dfs2id[a]
        for k in range(int(tree.mut_off[i]), int(tree.mut_off[i + 1])):
            if tree.mut_pos[k] >= 0:
                pos.append(int(tree.mut_pos[k])); node.append(int(dfs_end[a]) + 1); ext.append(True); owner.append(a)

    for d in range(tree.n_nodes):
        while open_ and dfs_end[open_[-1]] < d:
            close(open_.pop())
        i = dfs2id[d]
        mine = [int(tree.mut_pos[k]) for k in range(int(tree.mut_off[i]), int(tree.mut_off[i + 1])) if tree.mut_pos[k] >= 0]
        if not mine:
            continue
        for p in mine:
            pos.append(p); node.append(d); ext.append(False); owner.append(d)
        open_.append(d)
    while open_:
        close(open_.pop())
    return dict(pos=np.array(pos, np.int64), node=np.array(node, np.int64), exit=np.array(ext, bool),
                owner=np.array(owner, np.int64), n_nodes=tree.n_nodes)


def window_events(tree_or_stream, ws, we):
    """The sub-sequence of the stream with ws <= pos <= we (what k_epp_select_scatter writes for a group)."""
    st = tree_or_stream if isinstance(tree_or_stream, dict) else stream(tree_or_stream)
    keep = (st["pos"] >= ws) & (st["pos"] <= we)
    return dict(pos=st["pos"][keep], node=st["node"][keep], exit=st["exit"][keep], owner=st["owner"][keep],
                n_nodes=st["n_nodes"])


def chunks(n_events):
    """[e0, e1) of every piece of a window stream of n_events under chunk_events = 1024 (one empty piece for an empty
    stream, as groups[g].nchunks = max(1, ...) has it)."""
    n = max(1, -(-n_events // CHUNK_EVENTS))
    return [(c * CHUNK_EVENTS, min(n_events, (c + 1) * CHUNK_EVENTS)) for c in range(n)]


def chunk_node_ranges(wev):
    """Per chunk of a window stream the nodes [p0, p1) it credits (k_epp_sweep: p_prev .. p_end)."""
    n, N = len(wev["pos"]), wev["n_nodes"]
    out = []
    for c, (e0, e1) in enumerate(chunks(n)):
        p0 = 0 if c == 0 else int(wev["node"][e0])
        p1 = int(wev["node"][e1]) if e1 < n else N
        out.append((p0, p1))
    return out


def assert_default_chunking(n_max, ntiles):
    """chunk_events = max(1024, ceil(n_max / ceil(262144 / ntiles))) rounded up to 64 is 1024 whenever
    n_max * ntiles <= 1024 * 262144 (about 2.7e8).  WEPP_EPP_TARGET_JOBS must be unset: it is read once per process."""
    import os
    assert "WEPP_EPP_TARGET_JOBS" not in os.environ
    assert n_max * ntiles <= CHUNK_EVENTS * TARGET_JOBS, (n_max, ntiles)
    want_chunks = max(1, -(-TARGET_JOBS // ntiles))
    assert ((max(CHUNK_EVENTS, -(-n_max // want_chunks)) + 63) & ~63) == CHUNK_EVENTS


def group_streams(tree, pl):
    """Window stream of every group of a plan, and the check that the cuts are 1024 apart."""
    st = stream(tree)
    out = [window_events(st, int(pl["group_ws"][g]), int(pl["group_we"][g])) for g in range(pl["G"])]
    assert_default_chunking(max(len(w["pos"]) for w in out), pl["ntiles"])
    return out


def jobs(pl, streams):
    """Sweep jobs of a plan: chunks of every group times its tiles."""
    return sum(len(chunks(len(w["pos"]))) * int(pl["group_ntiles"][g]) for g, w in enumerate(streams))


def epp_list(out, r):
    return out["epp_nodes"][int(out["epp_off"][r]):int(out["epp_off"][r + 1])]


def exact_scores(oracle_out, degree, n_nodes):
    """score[n] = sum over the reads r whose EPP list holds n of degree_r / ((1 + max_parsimony_r) * multiplicity_r)
    (initial_filter.hpp:54-57) as fractions.Fraction, from the oracle's integer outputs alone, and n_contrib[n], the
    number of those reads.  Valid only where the oracle kept every list (multiplicity <= 2048)."""
    assert n_nodes <= ORACLE_LIST_CAP
    mp, mult, off = oracle_out["max_parsimony"], oracle_out["multiplicity"], oracle_out["epp_off"]
    assert (mult <= ORACLE_LIST_CAP).all() and (np.diff(off.astype(np.int64)) == mult).all()
    by_den = {}                                   # denominator -> integer numerators per node
    n_contrib = np.zeros(n_nodes, np.int64)
    deg_sum = np.zeros(n_nodes, np.int64)
    for r in range(len(mp)):
        nodes = epp_list(oracle_out, r).astype(np.int64)
        num = by_den.setdefault((1 + int(mp[r])) * int(mult[r]), np.zeros(n_nodes, np.int64))
        num[nodes] += int(degree[r])
        n_contrib[nodes] += 1
        deg_sum[nodes] += int(degree[r])
    score = [Fraction(0)] * n_nodes
    for den, num in by_den.items():
        for n in np.nonzero(num)[0]:
            score[n] += Fraction(int(num[n]), den)
    return score, n_contrib, deg_sum


def fx_bits(total_degree):
    """Bits behind the binary point of the library's 64-bit fixed point (epp_map_run)."""
    return min(52, 62 - int(total_degree).bit_length())


def score_bound(exact, n_contrib, total_degree):
    """Every read's delta is one double division, rounded once to a multiple of 2^-k; the sums are exact integers; the
    result is converted to double once: |got - exact| <= n_contrib * 2^-(k+1) + exact * 2^-51 (the second term is twice
    the two relative roundings of 2^-53 each, the factor 2 slack for their product terms)."""
    k = fx_bits(total_degree)
    return int(n_contrib) * Fraction(1, 2 ** (k + 1)) + exact * Fraction(1, 2 ** 51)


# ---------------------------------------------------------------------------------------------------------------
# small helpers of the builders
# ---------------------------------------------------------------------------------------------------------------
def _alts(r):
    return [b for b in (1, 2, 4, 8) if b != r]


def genotype_read(geno, ref, node, start, end, positions=None):
    """Entries of a read that shows node's genotype on [start, end] (or on `positions` only)."""
    g = geno[node]
    ps = sorted(p for p in g if start <= p <= end and (positions is None or p in positions))
    return [(p, ref[p], g[p], 0) for p in ps if g[p] != ref[p]]


def concat_reads(a, b):
    off = np.concatenate([a.read_off, b.read_off[1:] + a.read_off[-1]])
    return EppReads(off, np.concatenate([a.read_word, b.read_word]), np.concatenate([a.start, b.start]),
                    np.concatenate([a.end, b.end]), np.concatenate([a.degree, b.degree]))


def with_degrees(reads, degree):
    return EppReads(reads.read_off, reads.read_word, reads.start, reads.end, np.asarray(degree, np.int32))


def take_reads(base, idx, degree=None):
    """The reads idx of `base` (any order, repeats allowed) by array operations only."""
    idx = np.asarray(idx, np.int64)
    lens = np.diff(base.read_off.astype(np.int64))[idx]
    off = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    src = np.repeat(base.read_off[:-1].astype(np.int64)[idx], lens) + (np.arange(off[-1]) - np.repeat(off[:-1], lens))
    return EppReads(off.astype(np.uint32), base.read_word[src], base.start[idx], base.end[idx],
                    base.degree[idx] if degree is None else degree)


def tile_reads(rng, base, n_reads, max_degree=4):
    """n_reads reads drawn from the distinct reads of `base`, with degrees of their own."""
    return take_reads(base, rng.integers(0, base.n_reads, n_reads), rng.integers(1, max_degree + 1, n_reads).astype(np.int32))


def degrees_summing_to(rng, n, total, max_degree=4):
    """n degrees of 1..max_degree whose sum is exactly `total` (the last few reads take what is left)."""
    assert n <= total <= n * max_degree
    d = rng.integers(1, max_degree + 1, n).astype(np.int64)
    i = 0
    while d.sum() != total:
        step = int(np.sign(total - d.sum()))
        if 1 <= d[i % n] + step <= max_degree:
            d[i % n] += step
        i += 1
    return d.astype(np.int32)


def degrees_just_under_2_31(n):
    """Seven reads of degree 2^28 spread among reads of degree 1; one read takes the rest: the sum is 2^31 - 1
    (k = 31), below 2^31 because the per-bin counts are int as in the reference."""
    assert n >= 16
    d = np.ones(n, np.int64)
    big = np.linspace(0, n - 2, 7).astype(int)
    d[big] = 1 << 28
    d[n - 1] = (1 << 31) - 1 - (d.sum() - 1)
    assert d.sum() == (1 << 31) - 1 and d[n - 1] >= 1 and (d < (1 << 31)).all()
    return d.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# A. chunk cuts
# ---------------------------------------------------------------------------------------------------------------
CHUNK_GENOME = 60
_WIN_LO, _WIN_HI = 11, 50                       # the 40-position window the tree's mutations lie in
_ROOT_POS, _HUB1_POS, _HUB3_POS = 40, 30, (20, 21, 22)

# (root mutation, events of the whole stream, leaves under the one-mutation hub, tail leaves under the root).
# The stream is  [root] hub1 | A pairs | hub1 exit | hub3 x 3 | B pairs | hub3 exits x 3 | tail pairs | [root exit],
# 2 * root + 8 + 2 * leaves events in all (see chunk_tree); what every case shows is asserted in test_epp_cases.py.
CHUNK_CASES = {
    # without a root mutation
    "plain-1024": (0, 1024, 200, 1),            # one full chunk, no cut
    "plain-1026": (0, 1026, 200, 1),            # a second chunk of two events: the last tail leaf, between pairs
    "plain-2048": (0, 2048, 510, 1),            # hub3's enters at 1022..1024: one node index on both sides of the cut
    "plain-2050": (0, 2050, 600, 1),            # cuts at 1024 (inside a pair of an A leaf) and at 2048 (between pairs)
    # with one root mutation
    "root-1024": (1, 1024, 200, 1),
    "root-1026": (1, 1026, 200, 0),             # hub3's exits at 1022..1024, all at node index N: an empty last chunk
    "root-2048": (1, 2048, 510, 1),             # hub3's enters at 1023..1025
    "root-2050": (1, 2050, 600, 2),             # cut at 1024 between pairs, at 2048 inside a tail leaf's pair
}


def chunk_tree(root_mut, n_events, n_a, n_tail):
    """A star-like tree over a genome of 60: a root (one mutation in the `root` variants), two hubs below it -- hub1
    with one mutation and n_a leaves, hub3 with three mutations and the rest of the leaves (the two side by side
    rather than one below the other, so that hub3's three events can be put on a cut by the choice of n_a) -- and
    n_tail leaves on the root itself, last in pre-order, so that the last piece of a stream can hold a node.
    Every leaf carries one mutation, at positions cycling through the
    window 11..50 (the hubs' and the root's positions left out, so every parent allele is the reference's); the first
    leaf of hub1 and the last node carry alleles no other leaf has at their positions."""
    leaves = (n_events - 2 * root_mut - 8) // 2
    assert 2 * root_mut + 8 + 2 * leaves == n_events
    n_b = leaves - n_a - n_tail
    assert n_a >= 2 and n_b >= 2 and n_tail >= 0
    rng = np.random.default_rng(n_events * 2 + root_mut)
    ref = {p: 1 << int(rng.integers(0, 4)) for p in range(1, CHUNK_GENOME + 1)}
    leaf_pos = [p for p in range(_WIN_LO, _WIN_HI + 1) if p not in (_ROOT_POS, _HUB1_POS) + _HUB3_POS]
    parent, muts = [-1], [[(_ROOT_POS, ref[_ROOT_POS], _alts(ref[_ROOT_POS])[0])] if root_mut else []]
    hub1 = len(parent)
    parent.append(0); muts.append([(_HUB1_POS, ref[_HUB1_POS], _alts(ref[_HUB1_POS])[1])])
    n_leaf = 0

    def leaf(par, special=False):
        nonlocal n_leaf
        p = leaf_pos[n_leaf % len(leaf_pos)]
        a = _alts(ref[p])[2] if special else _alts(ref[p])[(n_leaf // len(leaf_pos)) % 2]
        parent.append(par); muts.append([(p, ref[p], a)])
        n_leaf += 1
        return len(parent) - 1

    first_a = leaf(hub1, special=True)
    for _ in range(n_a - 1):
        leaf(hub1)
    hub3 = len(parent)
    parent.append(0); muts.append([(p, ref[p], _alts(ref[p])[0]) for p in _HUB3_POS])
    last = None
    for i in range(n_b):
        last = leaf(hub3, special=(n_tail == 0 and i == n_b - 1))
    for i in range(n_tail):
        last = leaf(0, special=(i == n_tail - 1))
    tree = Tree.from_lists(parent, muts)
    # ids are pre-order indices here: children have larger ids than their parent and subtrees are contiguous
    assert (preorder(tree)[0] == np.arange(tree.n_nodes)).all()
    return tree, ref, dict(hub1=hub1, hub3=hub3, first_a=first_a, last=last, n_a=n_a, n_b=n_b, n_tail=n_tail)


def chunk_case(name, degrees=None):
    """Tree and 130 reads (three tiles of 64) of a chunk-cut case: 110 of epp_fuzz.random_epp_reads, then hand-made
    ones (their indices in `hand`).  All hand-made reads start at 1 or 2, so they share the first tile -- whose
    window is the whole genome, so that its group sweeps the whole stream -- with the earliest random reads."""
    root_mut, n_events, n_a, n_tail = CHUNK_CASES[name]
    tree, ref, nodes = chunk_tree(root_mut, n_events, n_a, n_tail)
    rng = np.random.default_rng(977 + n_events + root_mut)
    geno = epp_fuzz.genotypes(tree, ref)
    rnd = epp_fuzz.random_epp_reads(rng, tree, ref, CHUNK_GENOME, n_reads=110, geno=geno)
    G = CHUNK_GENOME
    hand, ents, start, end = {}, [], [], []

    def add(key, e, s, t):
        hand.setdefault(key, []).append(110 + len(ents))
        ents.append(e); start.append(s); end.append(t)

    for _ in range(3):
        add("everywhere", [], 1, _WIN_LO - 1)                      # no mutation of the tree in 1..10: every node is optimal
    for _ in range(3):
        add("whole", [], 1, G)                                     # the whole genome, the reference's bases
    for _ in range(3):
        add("last", genotype_read(geno, ref, nodes["last"], 1, G), 1, G)        # only the last node matches
    for _ in range(3):
        add("first", genotype_read(geno, ref, nodes["first_a"], 1, G), 1, G)    # only hub1's first leaf matches
    # hub1's subtree (hub3's) is optimal, but for the leaves that mutate a listed position again
    add("under_hub1", genotype_read(geno, ref, nodes["hub1"], 2, G, {_HUB1_POS}), 2, _HUB1_POS)
    add("under_hub1", genotype_read(geno, ref, nodes["hub1"], 2, G, {_HUB1_POS}), 2, G)
    add("under_hub3", genotype_read(geno, ref, nodes["hub3"], 2, G, set(_HUB3_POS)), 2, _HUB3_POS[-1])
    add("under_hub3", genotype_read(geno, ref, nodes["hub3"], 2, G, set(_HUB3_POS)), 2, G)
    add("under_hub3", genotype_read(geno, ref, nodes["hub3"], 2, G, set(_HUB3_POS[:2]) | {_ROOT_POS}), 2, G)
    add("under_hub3", [(_HUB3_POS[0], ref[_HUB3_POS[0]], 15, 1)], 2, G)         # an N on one of hub3's positions
    for _ in range(2):
        add("everywhere", [], 2, _WIN_LO - 1)
    hm = EppReads.from_lists(ents, start, end, rng.integers(1, 5, len(ents)).astype(np.int32))
    reads = concat_reads(rnd, hm)
    assert reads.n_reads == 130
    if degrees is not None:
        reads = with_degrees(reads, degrees)
    return dict(tree=tree, ref=ref, nodes=nodes, reads=reads, hand=hand, genome=CHUNK_GENOME, n_events=n_events,
                root_mut=root_mut)


# ---------------------------------------------------------------------------------------------------------------
# B. groups of several tiles
# ---------------------------------------------------------------------------------------------------------------
GROUP_GENOME = 3000
GROUP_CASES = {32769: (1, 2, 257, 1), 65537: (1, 3, 342, 2), 131073: (4, 2, 257, 1)}   # R: rpl, tpg, G, tiles of the last group
_group_base = {}


def group_tree_and_base():
    """A tree of 150 nodes with about 5 900 mutations all over a genome of 3000 (none masked: two per position, so that
    a group's stream is a few runs of 64 events and most reads have few optimal nodes, which keeps the CPU oracle's
    share of the 131 073-read case down) and 4000 distinct reads of 1..25 positions; built once and shared."""
    if not _group_base:
        rng = np.random.default_rng(20250)
        tree, ref = ft.random_tree(rng, n_nodes=150, genome=GROUP_GENOME, p_masked=0.0, p_root_masked=0.0, max_muts=80)
        assert (tree.mut_pos >= 0).all()
        base = epp_fuzz.random_epp_reads(rng, tree, ref, GROUP_GENOME, n_reads=4000, max_len=25)
        _group_base.update(tree=tree, ref=ref, base=base)
    return _group_base["tree"], _group_base["base"]


def group_case(n_reads):
    tree, base = group_tree_and_base()
    reads = tile_reads(np.random.default_rng(n_reads), base, n_reads)
    return dict(tree=tree, reads=reads, genome=GROUP_GENOME, rpl=GROUP_CASES[n_reads][0])


def hole_blocks(wev, tws, twe):
    """Of the runs of 64 events the sweep takes from a group's stream (from every chunk's start), those of which some
    events, but not a prefix, lie in the tile's window -- and those of which none does."""
    inside = (wev["pos"] >= tws) & (wev["pos"] <= twe)
    holes, empty = [], []
    for e0, e1 in chunks(len(inside)):
        for b0 in range(e0, e1, 64):
            m = inside[b0:min(e1, b0 + 64)]
            k = int(m.sum())
            if k == 0:
                empty.append(b0)
            elif not m[:k].all():
                holes.append(b0)
    return holes, empty


# ---------------------------------------------------------------------------------------------------------------
# C. selection
# ---------------------------------------------------------------------------------------------------------------
SKIP_GENOME = 600


def group_skip_case():
    """Six tiles of reads at one read per lane: the first read in the order spans nearly the whole genome, the others
    are short, so the groups' window ends are not monotone and a position of group 0 can belong to a later group and
    to none between them."""
    rng = np.random.default_rng(606)
    tree, ref = ft.random_tree(rng, n_nodes=200, genome=SKIP_GENOME, p_masked=0.0, p_root_masked=0.0, max_muts=6)
    geno = epp_fuzz.genotypes(tree, ref)
    short = epp_fuzz.random_epp_reads(rng, tree, ref, SKIP_GENOME, n_reads=6 * 64 + 15, max_len=8, geno=geno)
    # (a short read that starts at 1 would sort before the long one)
    short = take_reads(short, np.nonzero(short.start > 1)[0][:6 * 64 - 1])
    assert short.n_reads == 6 * 64 - 1
    keep_first = EppReads.from_lists([genotype_read(geno, ref, 57, 1, SKIP_GENOME - 10)], [1], [SKIP_GENOME - 10], [3])
    reads = concat_reads(short, keep_first)
    return dict(tree=tree, reads=reads, genome=SKIP_GENOME, long_read=reads.n_reads - 1)


SCAN_NODES = 130000         # nodes of the generated MAT of the select-scan case (see select_scan_case)


def select_scan_case():
    """A generated MAT with more than 131 072 non-masked mutations: its stream has more than 256 selection blocks of
    1024 events, so k_epp_select_scan goes round its loop more than once and carries the running count over."""
    import wepp_amd as w
    g = w.generate_tree(21, SCAN_NODES)
    reads = g.reads(22, 200, read_len=150, amplicon_len=400, amplicon_step=300, p_substitution=0.003, p_n=0.01,
                    windows=True, max_degree=5)
    return dict(tree=g.tree, reads=reads, genome=29903, gen=g)


def select_blocks(tree):
    return -(-2 * int((tree.mut_pos >= 0).sum()) // SEL_EVENTS)


# ---------------------------------------------------------------------------------------------------------------
# D. list cap
# ---------------------------------------------------------------------------------------------------------------
CAP_NODES = 40


def list_cap_case():
    """A tree of 40 nodes over a genome of 60 and 48 reads of three kinds, interleaved in window order inside one tile:
    every node optimal (a window that holds no mutation of the tree), exactly one node, exactly two (a node and its
    only child, whose own mutation lies outside the read's window)."""
    rng = np.random.default_rng(4040)
    ref = {p: 1 << int(rng.integers(0, 4)) for p in range(1, 61)}
    parent, muts = [-1], [[]]
    parent.append(0); muts.append([(20, ref[20], _alts(ref[20])[0])])            # node 1
    parent.append(1); muts.append([(45, ref[45], _alts(ref[45])[0])])            # node 2: differs from node 1 at 45 only
    pos = [p for p in range(11, 30) if p != 20]
    for i in range(CAP_NODES - 3):                                               # leaves on the root, one mutation each
        p = pos[i % len(pos)]
        parent.append(0); muts.append([(p, ref[p], _alts(ref[p])[i // len(pos)])])
    tree = Tree.from_lists(parent, muts)
    assert tree.n_nodes == CAP_NODES
    geno = epp_fuzz.genotypes(tree, ref)
    ents, start, end, kind = [], [], [], []
    free = [(1, 5), (2, 9), (3, 3), (4, 10), (5, 8), (6, 6), (7, 10), (8, 9), (31, 40), (32, 44), (33, 33), (46, 60),
            (47, 50), (52, 60), (31, 31), (34, 44)]
    for i in range(16):
        s, e = free[i]
        ents.append([]); start.append(s); end.append(e); kind.append(CAP_NODES)
        leaf = 3 + 2 * i
        ents.append(genotype_read(geno, ref, leaf, 1, 60)); start.append(1 + i % 10); end.append(30 + i % 14); kind.append(1)
        ents.append(genotype_read(geno, ref, 1, 1, 44)); start.append(1 + (i * 3) % 10); end.append(30 + (i * 5) % 14); kind.append(2)
    reads = EppReads.from_lists(ents, start, end, rng.integers(1, 5, len(ents)).astype(np.int32))
    return dict(tree=tree, reads=reads, genome=60, kind=np.array(kind), caps=(0, 1, CAP_NODES - 1, CAP_NODES, CAP_NODES + 1))


def cut_lists(want, cap):
    """The oracle's lists cut down to `cap` the way the library does (tests/test_epp_gpu.py::test_generated_trees)."""
    n = len(want["multiplicity"])
    keep = want["multiplicity"] <= cap
    off = np.zeros(n + 1, np.uint64)
    nodes = []
    for r in range(n):
        if keep[r]:
            nodes.append(epp_list(want, r))
        off[r + 1] = off[r] + (want["multiplicity"][r] if keep[r] else 0)
    out = dict(want)
    out["epp_off"] = off
    out["epp_nodes"] = np.concatenate(nodes) if nodes else np.zeros(0, np.uint32)
    return out, keep


# ---------------------------------------------------------------------------------------------------------------
# E. exact scores
# ---------------------------------------------------------------------------------------------------------------
DEGREE_TOTALS = {"k52": (1 << 10) - 1, "k51": 1 << 10, "k31": (1 << 31) - 1}


def degrees_for(which, n, seed):
    if which == "k31":
        return degrees_just_under_2_31(n)
    return degrees_summing_to(np.random.default_rng(seed), n, DEGREE_TOTALS[which], max_degree=15)


def fuzz_score_case(which):
    """A 600-read fuzz batch on a fuzz tree of 64 nodes, degrees summing to the total that sets the fixed point's scale."""
    rng = np.random.default_rng(600)
    tree, ref = ft.random_tree(rng, n_nodes=64, genome=60, p_masked=0.0, p_root_masked=0.0)
    reads = epp_fuzz.random_epp_reads(rng, tree, ref, 60, n_reads=600)
    return dict(tree=tree, reads=with_degrees(reads, degrees_for(which, 600, 601)), genome=60)


SPARSE_SIZES = (3, 5, 6, 7, 9, 11, 24, 48, 23, 37, 96, 13)


def sparse_score_case(which):
    """Haplotypes with ONE contributing read each, so that a single rounding shows: a root with a hub of every size in
    SPARSE_SIZES (the hub carries one mutation, its other nodes none) and a sink leaf.  Read j covers the position of
    hub j alone and shows its allele: it is optimal on that hub's subtree, multiplicity SPARSE_SIZES[j], degree 1 or 2
    -- a delta that is no multiple of 2^-k.  The sink's own reads carry the rest of the total degree."""
    rng = np.random.default_rng(3)
    ref = {p: 1 << int(rng.integers(0, 4)) for p in range(1, 61)}
    parent, muts, ents, start, end, degree = [-1], [[]], [], [], [], []
    for j, size in enumerate(SPARSE_SIZES):
        p = 5 + 2 * j
        hub = len(parent)
        parent.append(0); muts.append([(p, ref[p], _alts(ref[p])[0])])
        for _ in range(size - 1):
            parent.append(hub); muts.append([])
        ents.append([(p, ref[p], _alts(ref[p])[0], 0)]); start.append(p); end.append(p); degree.append(1 + j % 2)
    parent.append(0); muts.append([(50, ref[50], _alts(ref[50])[0])])
    rest = DEGREE_TOTALS[which] - sum(degree)
    big = (1 << 28) if which == "k31" else 100
    for d in [big] * 7 + [rest - 7 * big]:
        ents.append([(50, ref[50], _alts(ref[50])[0], 0)]); start.append(50); end.append(50); degree.append(d)
    assert min(degree) >= 1
    tree = Tree.from_lists(parent, muts)
    return dict(tree=tree, reads=EppReads.from_lists(ents, start, end, np.array(degree, np.int32)), genome=60)


def score_case(which, batch):
    if batch == "fuzz":
        return fuzz_score_case(which)
    if batch == "sparse":
        return sparse_score_case(which)
    return chunk_case(batch, degrees_for(which, 130, 131))


SCORE_BATCHES = ("fuzz", "plain-2050", "sparse")


def fixed_point_scores(oracle_out, degree, n_nodes, truncate=False):
    """The library's arithmetic restated on the oracle's integer outputs (k_epp_combine, k_epp_scan_apply): one double
    division per read, times 2^k, rounded to the nearest integer (truncate=True: toward zero, what the test must be
    able to tell from it), exact integer sums, one conversion to double."""
    import math
    k = fx_bits(int(np.asarray(degree, np.int64).sum()))
    acc = [0] * n_nodes
    for r in range(len(oracle_out["multiplicity"])):
        x = Fraction(float(degree[r]) / float((1 + int(oracle_out["max_parsimony"][r])) * int(oracle_out["multiplicity"][r]))) * 2 ** k
        fx = math.floor(x) if truncate else round(x)
        for n in epp_list(oracle_out, r):
            acc[int(n)] += fx
    return np.array([float(a) * 2.0 ** -k for a in acc])


# ---------------------------------------------------------------------------------------------------------------
# F. reads per lane, LDS limit
# ---------------------------------------------------------------------------------------------------------------
RPL_GENOME = 600


def rpl_switch_case(longest):
    """300 reads of which the longest has end - start = `longest` (383: WEPP_EPP_RPL=4 holds; 384: it falls back to 1)."""
    rng = np.random.default_rng(383)
    tree, ref = ft.random_tree(rng, n_nodes=120, genome=RPL_GENOME, p_masked=0.0, p_root_masked=0.0, max_muts=6)
    geno = epp_fuzz.genotypes(tree, ref)
    short = epp_fuzz.random_epp_reads(rng, tree, ref, RPL_GENOME, n_reads=299, max_len=120, geno=geno)
    s = 100
    long_ = EppReads.from_lists([genotype_read(geno, ref, 77, s, s + longest)], [s], [s + longest], [2])
    reads = concat_reads(short, long_)
    assert int((reads.end - reads.start).max()) == longest
    return dict(tree=tree, reads=reads, genome=RPL_GENOME)


LDS_GENOME = 6000


def lds_limit_spans():
    """The largest span = end - start whose plan stays within 150 KiB of LDS, and the smallest above."""
    span = 0
    while lds_bytes(span + 1) <= LDS_LIMIT:
        span += 1
    assert lds_bytes(span) <= LDS_LIMIT < lds_bytes(span + 1)
    return span, span + 1


def lds_limit_case(span):
    """One read of `span` = end - start on a genome of 6000, showing a node's genotype with a few N's."""
    rng = np.random.default_rng(6000)
    tree, ref = ft.random_tree(rng, n_nodes=100, genome=LDS_GENOME, p_masked=0.0, p_root_masked=0.0, max_muts=8)
    geno = epp_fuzz.genotypes(tree, ref)
    s = 17
    ents = genotype_read(geno, ref, 63, s, s + span)
    listed = {e[0] for e in ents}
    for p in (s, s + span // 2, s + span):
        if p not in listed:
            ents.append((p, ref[p], 15, 1))
    reads = EppReads.from_lists([sorted(ents)], [s], [s + span], [3])
    ordinary = epp_fuzz.random_epp_reads(rng, tree, ref, LDS_GENOME, n_reads=40, geno=geno)
    return dict(tree=tree, reads=reads, ordinary=ordinary, genome=LDS_GENOME)


# ---------------------------------------------------------------------------------------------------------------
# what an input shows, from the model and the oracle alone
# ---------------------------------------------------------------------------------------------------------------
# per chunk-cut case, what the sweep of its first group (the whole stream: its window is the whole genome) meets:
#   one_full_chunk     1024 events: one piece, filled to its last event
#   spans_chunks       some read's EPP list holds nodes of at least two pieces' node ranges
#   only_last          some read's optimum lies in the last piece alone (and there are several)
#   only_first         some read's optimum lies in the first piece alone
#   open_across_cut    some read is optimal on both nodes around a cut: its range is closed there and opened again
#   hub_straddle       hub3's events lie on both sides of a cut, with one node index
#   cut_in_pair        a cut between a leaf's enter and its exit
#   cut_between_nodes  a cut between the events of two different nodes
#   empty_last_chunk   the last piece holds events (all at node index N) but no node
CHUNK_SHOWS = {
    "plain-1024": {"one_full_chunk"},
    "plain-1026": {"spans_chunks", "only_last", "only_first", "open_across_cut", "cut_between_nodes"},
    "plain-2048": {"spans_chunks", "only_last", "only_first", "open_across_cut", "hub_straddle"},
    "plain-2050": {"spans_chunks", "only_last", "only_first", "open_across_cut", "cut_in_pair", "cut_between_nodes"},
    "root-1024": {"one_full_chunk"},
    "root-1026": {"only_first", "hub_straddle", "empty_last_chunk"},
    "root-2048": {"spans_chunks", "only_last", "only_first", "open_across_cut", "hub_straddle"},
    "root-2050": {"spans_chunks", "only_first", "open_across_cut", "cut_in_pair", "cut_between_nodes", "empty_last_chunk"},
}


def chunk_edges(case, want, rpl):
    """(what the first group's sweep meets, the plan, the groups' streams) of a chunk-cut case at WEPP_EPP_RPL=rpl;
    `want` is the oracle's result."""
    reads, nodes = case["reads"], case["nodes"]
    pl = plan(reads.start, reads.end, effective_rpl(reads.start, reads.end, rpl))
    gs = group_streams(case["tree"], pl)
    g0 = gs[0]
    assert (int(pl["group_ws"][0]), int(pl["group_we"][0])) == (1, case["genome"])
    n, N = len(g0["pos"]), g0["n_nodes"]
    ranges = chunk_node_ranges(g0)
    shows = set()
    if n == CHUNK_EVENTS and len(ranges) == 1:
        shows.add("one_full_chunk")
    if len(ranges) > 1 and ranges[-1][0] == ranges[-1][1]:
        shows.add("empty_last_chunk")
    for r in pl["order"][: int(pl["group_ntiles"][0]) * pl["tile_reads"]]:
        lst = epp_list(want, int(r)).astype(np.int64)
        assert len(lst) == want["multiplicity"][r]
        cs = {c for c, (a, b) in enumerate(ranges) if ((lst >= a) & (lst < b)).any()}
        if len(cs) >= 2:
            shows.add("spans_chunks")
        if len(ranges) > 1 and cs == {len(ranges) - 1}:
            shows.add("only_last")
        if len(ranges) > 1 and cs == {0}:
            shows.add("only_first")
        for a, _ in ranges[1:]:
            if 0 < a < N and a in lst and a - 1 in lst:
                shows.add("open_across_cut")
    hubs = (0, nodes["hub1"], nodes["hub3"])
    for _, e1 in chunks(n)[:-1]:
        a, b = e1 - 1, e1
        if g0["owner"][a] == g0["owner"][b] == nodes["hub3"] and g0["node"][a] == g0["node"][b]:
            shows.add("hub_straddle")
        if g0["owner"][a] == g0["owner"][b] and g0["owner"][a] not in hubs and not g0["exit"][a] and g0["exit"][b]:
            shows.add("cut_in_pair")
        if g0["owner"][a] != g0["owner"][b]:
            shows.add("cut_between_nodes")
    return shows, pl, gs


def group_edges(case):
    """For a several-tiles-per-group case: the plan, its groups' streams and one (group, tile, position, block) where
    the tile's window is smaller than the group's, a mutation of the tree lies in the group's window but outside the
    tile's, and a run of 64 events of the group's stream has some events, but not a prefix, inside the tile."""
    reads, tree = case["reads"], case["tree"]
    pl = plan(reads.start, reads.end, effective_rpl(reads.start, reads.end, case["rpl"]))
    st = stream(tree)
    gs = [window_events(st, int(pl["group_ws"][g]), int(pl["group_we"][g])) for g in range(pl["G"])]
    assert_default_chunking(max(len(w["pos"]) for w in gs), pl["ntiles"])
    mutated = np.unique(tree.mut_pos[tree.mut_pos >= 0])
    found, n_holes, n_empty = None, 0, 0
    for g in range(pl["G"]):
        gws, gwe = int(pl["group_ws"][g]), int(pl["group_we"][g])
        for t in range(int(pl["group_tile0"][g]), int(pl["group_tile0"][g] + pl["group_ntiles"][g])):
            tws, twe = int(pl["tile_ws"][t]), int(pl["tile_we"][t])
            if (tws, twe) == (gws, gwe):
                continue
            outside = mutated[(mutated >= gws) & (mutated <= gwe) & ((mutated < tws) | (mutated > twe))]
            holes, empty = hole_blocks(gs[g], tws, twe)
            n_holes += len(holes)
            n_empty += len(empty)
            if found is None and len(outside) and holes:
                found = dict(group=g, tile=t, position=int(outside[0]), block=holes[0])
    return dict(plan=pl, streams=gs, found=found, n_holes=n_holes, n_empty=n_empty)


def skip_edges(case):
    """For the group-skip case: the plan (one read per lane) and a mutated position that lies in group 0 and in a
    later group j, but in no group between them."""
    reads, tree = case["reads"], case["tree"]
    pl = plan(reads.start, reads.end, 1)
    ws, we = pl["group_ws"], pl["group_we"]
    mutated = np.unique(tree.mut_pos[tree.mut_pos >= 0])
    found = None
    for p in mutated:
        inside = np.nonzero((ws <= p) & (p <= we))[0]
        if len(inside) >= 2 and inside[0] == 0 and inside[1] >= 2:
            found = dict(position=int(p), later=int(inside[1]))
            break
    return dict(plan=pl, found=found)
