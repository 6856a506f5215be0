"""Inputs that put the pass-2 kernels (wepp_amd/csrc/pass2_kernels.hip: k_scores<false>, k_scores<true>, k_imputed,
k_excess) on both sides of their layout units, and the launch rule of launch_scores / launch_best_nodes restated.

A case is a tree, its calls and `facts`: statements about the INPUT, computed here from the flat image
(FlatView.get("blk_node0" | "blk_eoff" | "ev_word" | "ev_meta" | "cp_off" | "cp_word", stream)), the restated rule and
the oracle -- never from the library's results.  tests/test_pass2_cases.py holds every builder to its edge on the
CPU; tests/test_pass2_edges_gpu.py runs every call through the public API against the oracle.

  kind "scores"   calls = Batch: Mat.place_batch(per_node_scores=True), one wave per (read, chunk of the whole tree)
  kind "best"     calls = Batch: Mat.best_nodes_csr, one launch per plan over the plan's list of reads
  kind "imputed"  calls = (Batch, best_bfs_j): Mat.imputed_mutations, one thread per ambiguous entry
  kind "excess"   calls = (Batch, pair_read, pair_bfs_j): Mat.excess_mutations, one thread per pair

The block and target constants are read from the sources, so a case follows the kernels when they change."""
import functools
import os
import re

import numpy as np

import fuzz_trees as ft
import sweep_cases as sc
import sweep_model as sm
import wepp_amd as w
from wepp_amd import N, Reads, Tree

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "wepp_amd", "csrc")


def _const(name, *files):
    for f in files:
        m = re.search(r"\b%s\s*=\s*(\d+)u?\s*[,;]" % name, open(os.path.join(_CSRC, f)).read())
        if m:
            return int(m.group(1))
    raise AssertionError(name + " is not in " + ", ".join(files))


BLK_MAX_NODES = _const("BLK_MAX_NODES", "flatmat.hpp")             # nodes of a block: one per lane
BLK_MAX_EVENTS = _const("BLK_MAX_EVENTS", "flatmat.hpp")           # events of a block, unless one node has more
TARGET_WAVES = _const("PASS2_TARGET_WAVES", "pass2_kernels.hip", "device_mat.hpp")
MIN_CHUNK_BLOCKS = _const("PASS2_MIN_CHUNK_BLOCKS", "pass2_kernels.hip", "device_mat.hpp")
IMPUTED_THREADS, EXCESS_THREADS = 256, 128                          # launch_imputed / launch_excess: pairs per workgroup
WAVE = 64                                                           # lanes: nodes of a block, events / checkpoint words of a round
assert BLK_MAX_NODES == WAVE and BLK_MAX_EVENTS == 2 * WAVE, "the cases below are written for blocks of 64 nodes and 128 events"


def pass2_chunks(n_reads, NB, ncp, cp_stride, emit):
    """(nchunks, bpc) of a k_scores launch over n_reads reads: device_mat.hpp pass2_chunks.  emit: the list of optimal
    nodes (k_scores<true>), which takes no chunk shorter than MIN_CHUNK_BLOCKS blocks."""
    n = max(1, (TARGET_WAVES + n_reads - 1) // n_reads)
    if emit:
        n = min(n, max(1, NB // MIN_CHUNK_BLOCKS))
    n = min(n, ncp)
    bpc = (ncp + n - 1) // n * cp_stride
    return (NB + bpc - 1) // bpc, bpc


def geometry(flat, stream=None):
    g = sc.stream_geometry(flat, stream)
    return dict(NB=g["NB"], ncp=g["ncp"], cp_stride=g["cp_stride"])


def parse_debug_lines(err):
    """`[scores] n_reads=3 nchunks=607 bpc=2` and `[best_nodes] window 4: 17 reads nchunks=2 bpc=9` lines of stderr:
    ([(n_reads, nchunks, bpc)], [(kind, index, reads, nchunks, bpc)])."""
    scores = [tuple(int(x) for x in m) for m in re.findall(r"^\[scores\] n_reads=(\d+) nchunks=(\d+) bpc=(\d+)$", err, re.M)]
    best = [(k, int(i), int(c), int(n), int(b))
            for k, i, c, n, b in re.findall(r"^\[best_nodes\] (window|stream) (\d+): (\d+) reads nchunks=(\d+) bpc=(\d+)$", err, re.M)]
    return scores, best


# ---- reads ----------------------------------------------------------------------------------------------------------
class Batch:
    """The reads of one call: `lists` = the distinct reads, index[i] = which of them read i is (duplicates are cheap
    for the oracle and as good as any read for the launch rule)."""

    def __init__(self, lists, index=None):
        self.lists = [list(l) for l in lists]
        self.index = np.arange(len(lists)) if index is None else np.asarray(index, np.int64)
        one = Reads.from_lists(self.lists)
        k = np.diff(one.read_off.astype(np.int64))
        off = np.zeros(len(self.index) + 1, np.int64)
        np.cumsum(k[self.index], out=off[1:])
        words = [one.read_word[int(one.read_off[i]):int(one.read_off[i + 1])] for i in range(len(self.lists))]
        self.reads = Reads(off.astype(np.uint32), np.concatenate([words[i] for i in self.index] + [np.zeros(0, np.uint32)]))

    @property
    def n_reads(self):
        return len(self.index)


def cols(l):
    """A read as the four columns the oracle takes."""
    return tuple(list(c) for c in zip(*l)) if l else ([], [], [], [])


class Case:
    def __init__(self, name, kind, tree, calls, facts=None, info=None):
        self.name, self.kind, self.tree, self.calls = name, kind, tree, calls
        self.facts = facts or {}
        self.info = info or sc.TreeInfo(tree)

    def geom(self, stream=None):
        return geometry(self.info.flat, stream)

    def chunks(self, n_reads, stream=None, emit=None):
        return pass2_chunks(n_reads, emit=(self.kind == "best") if emit is None else emit, **self.geom(stream))


CASES, KINDS = {}, {}


def case(kind):
    """Registers a builder; its kind is known without building it (the test modules parametrise by it)."""
    def register(fn):
        CASES[fn.__name__] = functools.lru_cache(maxsize=None)(fn)
        KINDS[fn.__name__] = kind
        return CASES[fn.__name__]
    return register


def of_kind(kind):
    return sorted(n for n in CASES if KINDS[n] == kind)


# ---- what the flat image says about a read --------------------------------------------------------------------------
def cp_word_counts(flat, stream=None):
    """Checkpoint words per checkpoint: the mutations open where a chunk may start."""
    return np.diff(flat.get("cp_off", stream).astype(np.int64))


def cp_hits(flat, l, cpi, stream=None):
    """Indices, among the words of checkpoint cpi, of the words at positions the read lists."""
    off, word = flat.get("cp_off", stream), flat.get("cp_word", stream)
    listed = set(e[0] for e in l)
    return [i for i, x in enumerate(word[int(off[cpi]):int(off[cpi + 1])]) if int(x) & 0xFFFFF in listed]


def event_hits(flat, l, stream=None):
    """The events of the stream at positions the read lists: (block, index in the block, node offset, exit, leaf)."""
    word, meta, eo = flat.get("ev_word", stream), flat.get("ev_meta", stream), flat.get("blk_eoff", stream).astype(np.int64)
    listed = np.fromiter((e[0] for e in l), np.int64, len(l))
    pos = (word & 0xFFFFF).astype(np.int64)
    out = []
    for e in np.flatnonzero(np.isin(pos, listed) & (word != sc.W_PAD_POS)):
        b = int(np.searchsorted(eo, e, side="right")) - 1
        out.append((b, int(e - eo[b]), int(meta[e]) & 63, bool(int(word[e]) & sm.W_EXIT), bool(int(word[e]) & sm.W_LEAF)))
    return out


def block_shape(flat, stream=None):
    """(nodes, event slots, padding events) of every block."""
    n0, eo, word = flat.get("blk_node0", stream).astype(np.int64), flat.get("blk_eoff", stream).astype(np.int64), flat.get("ev_word", stream)
    return [(int(n0[b + 1] - n0[b]), int(eo[b + 1] - eo[b]), int((word[eo[b]:eo[b + 1]] == sc.W_PAD_POS).sum())) for b in range(len(n0) - 1)]


def block_of_bfs(flat, stream=None):
    """Block of the whole-tree stream that holds the node with BFS index j."""
    d2b, n0 = flat.get("dfs2bfs").astype(np.int64), flat.get("blk_node0", stream).astype(np.int64)
    blk = np.searchsorted(n0, np.arange(len(d2b)), side="right") - 1
    out = np.zeros(len(d2b), np.int64)
    out[d2b] = blk
    return out


def whole_tree_model(flat):
    fm = sm.FlatModel(flat)
    fm.cp_stride = int(flat.cp_stride)          # (the whole-tree stream has a checkpoint per seed chunk at least)
    return fm


def model_scores(fm, l, bpc):
    """Per-node scores of the Python model of the sweep, cut into chunks of bpc blocks like the launch: every chunk
    starts from its checkpoint's words.  Indexed by DFS index."""
    out = np.full(fm.N, -(1 << 30), np.int64)
    for b0 in range(0, fm.NB, bpc):
        fm.place(l, b0, min(fm.NB, b0 + bpc), node_scores=out)
    return out


def ref_of(p):
    return 1 << (p % 4)


def alt_of(p, k=1):
    return 1 << ((p + k) % 4)


def genotype_reads(info, nodes, seed, extra=3):
    """Reads that carry the alleles of the given nodes, with a few words besides."""
    rng = np.random.default_rng(seed)
    pool = list(range(1, info.max_pos + 1))
    return [sc.node_read(info, n, len(info.genotype(n)) + extra, rng, pool) for n in nodes]


# =====================================================================================================================
# k_scores<false>: per-node scores
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def small_tree():
    """About 100 nodes: two blocks."""
    g = w.generate_tree(5, 100, genome_len=300, p_ambiguous=0.02, p_masked_node=0.02, root_mutations=1)
    return sc.TreeInfo(g.tree)


def _varied_reads(info, n, seed):
    """n distinct reads of 0 - 8 words following nodes of the tree, the empty read and an all-missing one among them."""
    lists = sc.node_batch(info, [1 + i % 8 for i in range(n - 2)], seed)
    p = info.mutated[:3]
    return lists + [[], [(q, info.ref(q), N, 1) for q in p]]


@case("scores")
def chunks_one():
    """TARGET_WAVES reads on a tree of two blocks: one chunk; one read fewer: two."""
    info = small_tree()
    lists = _varied_reads(info, 32, 11)
    calls = [Batch(lists, np.arange(n) % len(lists)) for n in (TARGET_WAVES, TARGET_WAVES - 1)]
    return Case("chunks_one", "scores", info.tree, calls, info=info)


@case("scores")
def chunks_per_checkpoint():
    """One read per call on a stream with a checkpoint per block: every chunk is one block.  The empty read, a read
    whose entries are all missing, and one that follows a node."""
    info = sc.base()
    p = info.mutated[5:60:6]
    lists = [[], [(q, info.ref(q), N, 1) for q in p]] + genotype_reads(info, [info.tree.n_nodes - 7], 12)
    return Case("chunks_per_checkpoint", "scores", info.tree, [Batch([l]) for l in lists], info=info)


def ragged_counts(geom, emit=False):
    """The smallest read counts for which the rule leaves a last chunk of exactly one block, and none shorter than
    the others, with chunks of two blocks at least."""
    one = full = None
    for n in range(1, TARGET_WAVES + 1):
        nchunks, bpc = pass2_chunks(n, emit=emit, **geom)
        if bpc < 2 or nchunks < 2:
            continue
        if one is None and geom["NB"] % bpc == 1:
            one = n
        if full is None and geom["NB"] % bpc == 0:
            full = n
    assert one is not None and full is not None, geom
    return one, full


@case("scores")
def chunks_ragged():
    """Read counts for which NB % bpc == 1 (a last chunk of one block) and NB % bpc == 0."""
    info = sc._grown(2062)
    lists = _varied_reads(info, 16, 13)
    one, full = ragged_counts(geometry(info.flat))
    calls = [Batch(lists, np.arange(n) % len(lists)) for n in (one, full)]
    return Case("chunks_ragged", "scores", info.tree, calls, facts=dict(counts=(one, full)), info=info)


@functools.lru_cache(maxsize=None)
def bushy_tree():
    """14 000 nodes with seven mutations on average: blocks fill up with events, not nodes -- more than 1024 of them,
    so the whole-tree stream has a checkpoint every second block."""
    tree, _ = ft.random_tree(np.random.default_rng(3), n_nodes=14000, genome=4000, max_muts=14, p_masked=0.002, p_root_masked=0.0)
    return sc.TreeInfo(tree)


@case("scores")
def stride_2():
    """cp_stride == 2: three reads, a chunk per checkpoint, each of two blocks; chunks that start at a multiple of bpc
    and not of one block, the last one ragged.  The reads follow deep nodes: the positions they list are open at
    chunk starts with a non-zero enter_delta."""
    info = bushy_tree()
    flat = info.flat
    d2i, n0 = flat.get("dfs2id"), flat.get("blk_node0")
    NB = len(n0) - 1
    # the node in front of a chunk start in the middle of the stream, one near its end, and a deep one anywhere
    depth = np.zeros(info.tree.n_nodes, np.int64)
    for i in range(1, info.tree.n_nodes):
        depth[i] = depth[info.tree.parent[i]] + 1
    nodes = [int(d2i[int(n0[2 * (NB // 4)]) - 1]), int(d2i[int(n0[NB - 1]) - 1]), int(np.argmax(depth))]
    lists = genotype_reads(info, nodes, 14)
    fm = whole_tree_model(flat)
    nchunks, bpc = pass2_chunks(3, emit=False, **geometry(flat))
    moved = [sum(1 for b0 in range(bpc, NB, bpc) if fm.chunk_start_c(l, b0) != fm._c_none(l)) for l in lists]
    return Case("stride_2", "scores", info.tree, [Batch(lists)], facts=dict(chunk_starts_moved=moved), info=info)


def chain(n, extra_at=(), first=100):
    """A chain of n nodes: node d mutates position first + d away from the reference (the nodes in extra_at one more
    position, 50 000 + d), the last node is its only leaf."""
    muts = []
    for d in range(n):
        p = first + d
        m = [(p, ref_of(p), ref_of(p), alt_of(p))]
        if d in extra_at:
            m.append((50000 + d, ref_of(50000 + d), ref_of(50000 + d), alt_of(50000 + d)))
        muts.append(m)
    return Tree.from_lists([-1] + list(range(n - 1)), muts)


def _deep_checkpoint(i):
    tree = chain(200, ((), (5,))[i])
    l = [(100 + d, ref_of(100 + d), alt_of(100 + d), 0) for d in (10, 70, 130, 195)] + [(3000, ref_of(3000), alt_of(3000), 0)]
    return Case("deep_checkpoint_%d" % i, "scores", tree, [Batch([l, l[1:3]])])


@case("scores")
def deep_checkpoint_0():
    """A chain of 200 nodes: a chunk start has as many checkpoint words as mutations are open above it -- 64, 128 and
    192.  The read lists the positions of nodes 10, 70 and 130 with their alleles (words of the first, second and
    third round of 64 lanes) and of node 195, which no checkpoint holds."""
    return _deep_checkpoint(0)


@case("scores")
def deep_checkpoint_1():
    """The same chain with a second mutation at node 5: 65, 129 and 193 checkpoint words."""
    return _deep_checkpoint(1)


HEAVY = 70      # mutations of the two heavy nodes of block_tree(): more than 64, so 2 * HEAVY events exceed a block


@functools.lru_cache(maxsize=None)
def block_tree():
    """A hand-made tree, ids in pre-order (DFS index == id), every node but the root's grandchildren a child of the root:
      block 0  the root (two mutations) and 63 leaves of one mutation: 64 nodes, 65 events padded to 66;
      block 1  64 leaves of one mutation: 64 events, one round;
      block 2  64 leaves of two mutations: 128 events, two full rounds;
      block 3  X, an internal node of HEAVY mutations, and its two leaves;
      block 4  Y alone: the HEAVY exit events of X and its own HEAVY enter events, more than 128;
      block 5  Y's leaf, then W whose first events are Y's exits, and 40 leaves; block 6: 64 leaves more.
    Every mutation has a position of its own: node i's k-th mutation sits at 1000 * k + i (the heavy ones from 10 000 and 20 000 on)."""
    parent, muts = [-1], [[(1, ref_of(1), ref_of(1), alt_of(1)), (2, ref_of(2), ref_of(2), alt_of(2))]]

    def leaf(par, k=1):
        i = len(parent)
        parent.append(par)
        muts.append([(p, ref_of(p), ref_of(p), alt_of(p)) for p in (1000 * (j + 1) + i for j in range(k))])
        return i

    def heavy(par, first):
        i = len(parent)
        parent.append(par)
        muts.append([(first + j, ref_of(first + j), ref_of(first + j), alt_of(first + j)) for j in range(HEAVY)])
        return i

    for _ in range(63):
        leaf(0)
    for _ in range(64):
        leaf(0)
    for _ in range(64):
        leaf(0, 2)
    x = heavy(0, 10000)
    leaf(x), leaf(x)
    y = heavy(0, 20000)
    leaf(y)
    wn = leaf(0)
    for _ in range(40 + 64):
        leaf(0)
    return sc.TreeInfo(Tree.from_lists(parent, muts)), dict(x=x, y=y, w=wn)


@case("scores")
def block_edges():
    """One read that lists: a root mutation; the mutation of the node at offset 63 of block 0 (event 64 of 65: the
    second round, next to the padding event); a mutation in the one round of block 1; mutations in both rounds of
    block 2; Y's last mutation (an enter event beyond the 128th of a one-node block, and an exit event in front of W
    whose net the later blocks inherit).  Alone (a chunk per block: the net crosses chunk boundaries through the
    checkpoints), TARGET_WAVES times (one chunk: carried from block to block) and in between."""
    info, who = block_tree()
    m = lambda node, j=0: info.muts(node)[j]
    pick = [m(0, 1), m(63), m(64 + 10), m(128 + 3, 0), m(128 + 60, 1), m(who["y"], HEAVY - 1), m(who["x"], 3)]
    special = sorted((p, rf, mu, 0) for p, rf, _, mu in pick)
    others = [sorted((p, rf, rf if i % 2 else mu, 0) for i, (p, rf, _, mu) in enumerate(pick)),
              special[:3] + [(special[3][0], special[3][1], N, 1)]]
    lists = [special] + others
    calls = [Batch([special]), Batch(lists), Batch(lists, np.arange(TARGET_WAVES // 2) % 3), Batch(lists, np.arange(TARGET_WAVES) % 3)]
    return Case("block_edges", "scores", info.tree, calls, facts=dict(who=who), info=info)


@functools.lru_cache(maxsize=None)
def hand_tree():
    """About 60 nodes, ids in pre-order.  Root with two mutations; position 10 mutated three times down the path
    1 - 2 - 3 (forward at 1, back to the reference at 2, which is masked, forward to another allele at 3) and back
    again at the leaf 5; node 6, internal, with two mutations; a masked leaf 9; positions 75 and 76 mutated nowhere."""
    r = ref_of
    parent = [-1, 0, 1, 2, 3, 3, 1, 6, 6, 0]
    muts = [
        [(1, r(1), r(1), alt_of(1)), (2, r(2), r(2), alt_of(2))],
        [(10, r(10), r(10), alt_of(10))],
        [(-1, 0, 0, 0), (10, r(10), alt_of(10), r(10))],
        [(10, r(10), r(10), alt_of(10, 2)), (11, r(11), r(11), alt_of(11))],
        [(12, r(12), r(12), alt_of(12))],
        [(10, r(10), alt_of(10, 2), r(10))],
        [(20, r(20), r(20), alt_of(20)), (21, r(21), r(21), alt_of(21))],
        [(22, r(22), r(22), alt_of(22))],
        [(20, r(20), alt_of(20), r(20)), (23, r(23), r(23), alt_of(23))],
        [(-1, 0, 0, 0), (30, r(30), r(30), alt_of(30))],
    ]
    rng = np.random.default_rng(21)
    geno = [None] * 60
    for i in range(60):
        if i >= len(muts):
            parent.append(int(rng.choice([x for x in range(i) if x not in (4, 5, 7, 8, 9)])))      # (those stay leaves)
        g = dict(geno[parent[i]]) if i else {}
        if i >= len(muts):
            ml = []
            for p in sorted(set(int(x) for x in rng.integers(1, 71, size=int(rng.integers(0, 4))))):
                cur = g.get(p, r(p))
                mu = cur
                while mu == cur:
                    mu = 1 << int(rng.integers(0, 4))
                ml.append((p, r(p), cur, mu))
            muts.append(ml)
        for p, _, _, mu in muts[i]:
            if p >= 0:
                g[p] = mu
        geno[i] = g
    return sc.TreeInfo(Tree.from_lists(parent, muts))


def node_state(flat, l, node):
    """(touched, masked, leaf, nmut, ncom) of a node for a read, as k_scores sees them: the static counts of nstat and
    what the read's words at the node's own positions change (own_adjust)."""
    d = int(np.flatnonzero(flat.get("dfs2id") == node)[0])
    st = int(flat.get("nstat")[d])
    woff, words = flat.get("node_woff"), flat.get("words")
    Sd = {e[0]: e for e in l}
    ncom, touched = (st >> 14) & sm.NS_CNT, False
    for x in range(int(woff[d]), int(woff[d + 1])):
        s = Sd.get(int(words[x]) & 0xFFFFF)
        if s is not None:
            touched = True
            ncom += sm.own_adjust(words[x], s)[1]
    return dict(touched=touched, masked=bool(st & sm.NS_MASKED), leaf=bool(st & sm.NS_LEAF), nmut=st & sm.NS_CNT, ncom=ncom)


@case("scores")
def eligibility():
    """Reads that touch a masked node; a leaf whose only shared mutation (a back-mutation to the reference) the read
    contradicts, so its ncom goes to 0; an internal node all of whose mutations the read shares (ncom == nmut) and one
    none of whose it shares (ncom == 0 < nmut: it does not compete, its score is reported one higher)."""
    info = hand_tree()
    r = ref_of
    lists = [
        [(30, r(30), alt_of(30), 0)],                                              # the masked leaf 9
        [(10, r(10), alt_of(10, 3), 0)],                                           # leaf 5 (and the masked 2): back-mutations contradicted
        [(20, r(20), alt_of(20), 0), (21, r(21), alt_of(21), 0)],                  # node 6: both shared
        [(20, r(20), alt_of(20, 2), 0), (21, r(21), r(21), 0)],                    # node 6: neither shared
        [(10, r(10), r(10), 0), (20, r(20), N, 1), (30, r(30), r(30) | alt_of(30), 0)],
    ]
    return Case("eligibility", "scores", info.tree, [Batch(lists)], info=info)


# =====================================================================================================================
# k_scores<true>: all optimal nodes.  A call: (Batch, crowns) -- work skipping on or off for the routing
# =====================================================================================================================
STAR_LEAVES = 3000


@functools.lru_cache(maxsize=None)
def star_tree():
    """A root without mutations and STAR_LEAVES leaves that all carry the same mutation at position 10; the last leaf
    one more at position 20."""
    a = (10, ref_of(10), ref_of(10), alt_of(10))
    muts = [[]] + [[a] for _ in range(STAR_LEAVES)]
    muts[-1] = [a, (20, ref_of(20), ref_of(20), alt_of(20))]
    return sc.TreeInfo(Tree.from_lists([-1] + [0] * STAR_LEAVES, muts))


@case("best")
def ties_span_chunks():
    """A read that shares the leaves' mutation: every leaf is optimal, ties in every chunk.  Beside it a
    read that shares the last leaf's second mutation too (one optimal node, in the last block of the last chunk) and
    the empty read (the root alone).  Work skipping off: one plan on the whole-tree stream, its chunk count set by
    the NB / 8 cap."""
    info = star_tree()
    lists = [[(10, ref_of(10), alt_of(10), 0)], [(10, ref_of(10), alt_of(10), 0), (20, ref_of(20), alt_of(20), 0)], []]
    return Case("ties_span_chunks", "best", info.tree, [(Batch(lists), False), (Batch(lists), True), (Batch(lists[:1]), False)], info=info)


@case("best")
def nb_over_8():
    """A stream of fewer than 8 blocks: the cap gives one chunk whatever the reads."""
    info = small_tree()
    lists = _varied_reads(info, 7, 31)
    return Case("nb_over_8", "best", info.tree, [(Batch(lists), False), (Batch(lists), True)], info=info)


@case("best")
def many_reads_few_ties():
    """TARGET_WAVES reads (duplicates of 48): with work skipping off one list and one chunk; with it on the reads
    part into the plans of several streams, every list a strict subset of the call's reads."""
    info = sc.base()
    lists = _varied_reads(info, 48, 32)
    b = Batch(lists, np.arange(TARGET_WAVES) % len(lists))
    tm = sm.TieredModel(info.flat)
    return Case("many_reads_few_ties", "best", info.tree, [(b, False), (b, True)],
                facts=dict(routes=sorted(set(tm.route(l) for l in lists))), info=info)


@functools.lru_cache(maxsize=None)
def window_tree():
    """9 000 nodes on a 29.9 kb genome: crowns tree-wide, and genome windows whose candidates are a crown."""
    return w.generate_tree(303, 9000, genome_len=29903, p_ambiguous=0.02, p_masked_node=0.01, root_mutations=0, p_back_mutation=0.05)


@case("best")
def plans_mixed():
    """Short reads, 900-base reads that stay inside a genome window, and reads put together from four distant short
    ones, in one call: plans on window crowns, on tree-wide crowns and on the whole tree."""
    g = window_tree()
    info = sc.TreeInfo(g.tree)
    short = g.reads(72, 150, p_substitution=0.004, p_n=0.02, p_iupac=0.1)
    long_ = g.reads(73, 40, read_len=900, amplicon_len=1000, amplicon_step=700, p_substitution=0.05, p_n=0.02, p_iupac=0.1)
    noisy = g.reads(74, 40, p_substitution=0.03, p_n=0.02)
    noisy = sc.read_lists(noisy)
    # reads that leave their genome window, with more words than any crown's bound: the whole-tree stream
    spanning = [sorted(noisy[i] + noisy[i + 10] + noisy[i + 20] + noisy[i + 30]) for i in range(10)]
    spanning = [l for l in spanning if len(set(e[0] for e in l)) == len(l)]
    lists = sc.read_lists(short) + sc.read_lists(long_) + noisy + spanning
    tm = sm.TieredModel(info.flat)
    last = info.flat.n_streams - 1
    in_window = [l for l in lists if len(l) > sc.WIN_MIN_ENTRIES and l[-1][0] < l[0][0] // sc.WIN_STRIDE * sc.WIN_STRIDE + sc.WIN_SIZE]
    facts = dict(routes=sorted(set(tm.route(l) for l in lists)), in_window=len(in_window),
                 window_crowns=int(info.flat.stats.n_window_streams_crown),
                 whole_tree=sum(1 for l in spanning if l[-1][0] - l[0][0] >= sc.WIN_SIZE and tm.route(l) == last))
    return Case("plans_mixed", "best", info.tree, [(Batch(lists), True), (Batch(lists), False)], facts=facts, info=info)


# =====================================================================================================================
# k_imputed / k_excess
# =====================================================================================================================
def ambiguous_entries(l):
    """The entries k_imputed gets a thread for: not missing, more than one allele."""
    return [e for e in l if not e[3] and e[2] & (e[2] - 1)]


def _amb(p, with_ref=True):
    return (p, ref_of(p), (ref_of(p) if with_ref else alt_of(p, 2)) | alt_of(p), 0)


@case("imputed")
def pairs_256():
    """Calls with 255, 256 and 257 ambiguous entries in all (one workgroup less a thread, exactly one, one thread
    into the second); reads without such an entry first, in the middle and last.  And a call without any."""
    info = hand_tree()
    n = info.tree.n_nodes
    plain = [(12, ref_of(12), alt_of(12), 0), (40, ref_of(40), N, 1)]               # (a missing N is no ambiguous entry)
    five = lambda i: sorted([_amb(1 + (i * 5 + j) % 70, (i + j) % 3 != 0) for j in range(5)] + ([(75, ref_of(75), ref_of(75), 0)] if i % 2 else []))
    calls = []
    for total in (255, 256, 257):
        lists = [plain] + [five(i) for i in range(25)] + [[]] + [five(i) for i in range(25, 51)] + [[_amb(10), _amb(20, False)][:total - 255], plain]
        assert sum(len(ambiguous_entries(l)) for l in lists) == total
        calls.append((Batch(lists), np.array([(7 * i) % n for i in range(len(lists))], np.uint32)))
    calls.append((Batch([plain, [], plain]), np.array([3, 0, n - 1], np.uint32)))
    return Case("pairs_256", "imputed", info.tree, calls, info=info)


@functools.lru_cache(maxsize=None)
def bare_root_tree():
    """A fuzz tree of 50 nodes whose root has no mutation: the empty read lists nothing there."""
    tree, ref = ft.random_tree(np.random.default_rng(41), n_nodes=50, root_muts=False, p_root_masked=0.0)
    return sc.TreeInfo(tree), ref


@case("excess")
def pairs_128():
    """Calls of 127, 128 and 129 (read, node) pairs; pair 5 repeats pair 4, pair 7 -- the empty read at the bare root
    -- lists nothing between two pairs that do.  And a call of such pairs only: a total of 0."""
    info, ref = bare_root_tree()
    n = info.tree.n_nodes
    rng = np.random.default_rng(42)
    lists = [[]] + [ft.random_sample(rng, ref) for _ in range(9)]
    calls = []
    for total in (127, 128, 129):
        pr = np.array([1 + i % 9 for i in range(total)], np.uint32)
        pj = np.array([(11 * i + 3) % n for i in range(total)], np.uint32)
        pr[5], pj[5] = pr[4], pj[4]
        pr[7], pj[7] = 0, 0
        calls.append((Batch(lists), pr, pj))
    calls.append((Batch(lists), np.zeros(3, np.uint32), np.zeros(3, np.uint32)))
    return Case("pairs_128", "excess", info.tree, calls, info=info)


def every_node_reads(info):
    r = ref_of
    rng = np.random.default_rng(43)
    lists = [
        # position 10 (three times on the path 1 - 2 - 3), node 6's own mutation at 20 shared and at 21 not, positions
        # nobody mutates with and without the reference allele in the code
        [_amb(10), (20, r(20), alt_of(20) | alt_of(20, 2), 0), (21, r(21), r(21) | alt_of(21, 2), 0), _amb(75), _amb(76, False)],
        [(10, r(10), alt_of(10) | alt_of(10, 2), 0), (11, r(11), N, 1), (30, r(30), r(30) | alt_of(30), 0)],
        [(1, r(1), alt_of(1), 0), (2, r(2), r(2) | alt_of(2), 0), (10, r(10), alt_of(10, 2), 0)],
        [],
    ]
    for _ in range(6):
        # eight words each: half of them ambiguity codes, some missing
        l = []
        for p in sorted(set(int(x) for x in rng.integers(1, 77, size=8))):
            u = rng.random()
            a = int(rng.integers(1, 16)) if u < 0.5 else N if u < 0.65 else 1 << int(rng.integers(0, 4))
            l.append((p, r(p), a, 1 if 0.5 <= u < 0.65 else 0))
        lists.append(l)
    return lists


def _every_pair(info, lists):
    n = info.tree.n_nodes
    return np.repeat(np.arange(len(lists)), n), np.tile(np.arange(n), len(lists))


@case("imputed")
def every_node_imputed():
    """wepp_imputed_mutations for every (read, node) pair of the hand-made tree: every read once per node."""
    info = hand_tree()
    lists = every_node_reads(info)
    pr, pj = _every_pair(info, lists)
    return Case("every_node_imputed", "imputed", info.tree, [(Batch(lists, pr), pj.astype(np.uint32))], info=info)


@case("excess")
def every_node_excess():
    """wepp_excess_mutations for every (read, node) pair of the hand-made tree."""
    info = hand_tree()
    lists = every_node_reads(info)
    pr, pj = _every_pair(info, lists)
    return Case("every_node_excess", "excess", info.tree, [(Batch(lists), pr.astype(np.uint32), pj.astype(np.uint32))], info=info)


DEEP, DEEP_P = 300, 1000


@functools.lru_cache(maxsize=None)
def descending_chain(rising=False):
    """A chain of DEEP nodes, node d mutating position DEEP_P - d: the deeper, the lower (rising: DEEP_P + d)."""
    ps = [DEEP_P + d if rising else DEEP_P - d for d in range(DEEP)]
    return sc.TreeInfo(Tree.from_lists([-1] + list(range(DEEP - 1)), [[(p, ref_of(p), ref_of(p), alt_of(p))] for p in ps]))


def _deep_excess(name, rising):
    info = descending_chain(rising)
    lists = [[(2000, ref_of(2000), alt_of(2000), 0), (2001, ref_of(2001), N, 1)], []]
    nodes = [DEEP - 1, 0, DEEP // 2]
    pr = np.array([0, 0, 0, 1, 1, 1], np.uint32)
    pj = np.array(nodes + nodes, np.uint32)
    return Case(name, "excess", info.tree, [(Batch(lists), pr, pj)], info=info)


@case("excess")
def deep_descending_excess():
    """The reads list none of the chain's positions: every mutation on the path above the chosen node is a
    back-mutation of part (2) of k_excess.  Node d mutates position DEEP_P - d, so the climb meets the positions in
    ascending order and appends each.  The chosen nodes: the deepest, the root and one in the middle, for a read of
    two words and for the empty read."""
    return _deep_excess("deep_descending_excess", False)


@case("excess")
def deep_rising_excess():
    """The same chain with node d at DEEP_P + d: the climb meets the positions in descending order and inserts every
    back-mutation at the front, moving all it has."""
    return _deep_excess("deep_rising_excess", True)


@case("imputed")
def deep_descending_imputed():
    """One ambiguous entry at the position only the root mutates: the thread climbs the whole chain to find it."""
    info = descending_chain()
    l = [_amb(DEEP_P, False), (2000, ref_of(2000), alt_of(2000), 0)]
    return Case("deep_descending_imputed", "imputed", info.tree, [(Batch([l], [0, 0, 0]), np.array([DEEP - 1, 0, DEEP // 2], np.uint32))], info=info)


# ---- the oracle's answers -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_tree(name):
    import oracle_bridge
    return oracle_bridge.OracleTree(CASES[name]().tree)


def _placer(name):
    """The faithful restatement on small trees, the incremental checker (pinned to it by tests/test_incremental.py) on
    the large ones."""
    ot = oracle_tree(name)
    return ot.incremental() if ot.n > 5000 else ot


@functools.lru_cache(maxsize=None)
def want_scores(name, call):
    """[distinct reads, N] per-node scores by BFS index."""
    c = CASES[name]()
    pl = _placer(name)
    return np.stack([pl.place_sample(*cols(l), per_node_scores=True)["node_scores"] for l in c.calls[call].lists])


@functools.lru_cache(maxsize=None)
def want_best(name, call):
    """Per distinct read: (score, num_best, sorted BFS indices of the optimal nodes)."""
    c = CASES[name]()
    pl = _placer(name)
    out = []
    for l in c.calls[call][0].lists:
        r = pl.place_sample(*cols(l), want_best_vec=True)
        out.append((int(r["score"]), int(r["num_best"]), r["best_j_vec"].astype(np.uint32)))
    return out


@functools.lru_cache(maxsize=None)
def want_imputed(name, call):
    c = CASES[name]()
    ot = oracle_tree(name)
    b, bj = c.calls[call]
    return [ot.imputed_at_node(*cols(b.lists[int(i)]), int(j)) for i, j in zip(b.index, bj)]


@functools.lru_cache(maxsize=None)
def want_excess(name, call):
    c = CASES[name]()
    ot = oracle_tree(name)
    b, pr, pj = c.calls[call]
    return [ot.excess_at_node(*cols(b.lists[int(b.index[int(r)])]), int(j)) for r, j in zip(pr, pj)]
