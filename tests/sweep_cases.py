"""Inputs that put the tile sweeps (wepp_amd/csrc/sweep_kernels.hip) on both sides of their layout units, and the
launch rule of wepp_place_batch restated in plain Python.

Two halves:
  * plan arithmetic -- tile_reads, takes_table, ent_cap, key_cap, chunks, finalize_lanes_per_read: the rule of
    launch_plan.hpp (plan_launches) and device_mat.hpp written again as pure functions.  The GPU tests compare the
    library's `[plan]` lines (WEPP_DEBUG_PLANS=1) with predict_plan().
  * builders -- CASES[name]() returns a Case: tree, reads, the knobs that send the reads to the sweep in question and
    `facts`, statements about the INPUT (entry counts, hit events per block of the flat image, positions against the
    tile's smallest one, chunk lengths ...) computed here from the flat image and the oracle, never from the library's
    placement results.  tests/test_sweep_cases.py holds every builder to its edge; tests/test_sweep_edges_gpu.py runs
    them on the device.

List order of a plan: k_route hands every routing block a contiguous slice of the reads and up to 16 384 reads of a
call sit in one wave per block, so a plan's list keeps the batch's order; from SORT_MIN_READS reads on the whole-tree
stream the list is sorted (stably) by first listed position.  tiles_of() restates that, and the cases stay below
16 384 reads."""
import functools

import numpy as np

import sweep_model as sm
import wepp_amd as w
from wepp_amd import A, C, G, T, N, Reads, Tree

# ---- device_mat.hpp / sweep_kernels.hip ----------------------------------------------------------------------------
MAX_TILE_ENTRIES = 8192
DENSE_MAX_POS = (1 << 19) - 1          # position field of a dense key that matches no event
DENSE_MIN_READ_WORDS = 16
DENSE_WINDOW = 4096
DENSE_MIN_HITS = 3
DENSE_WAVES_PER_WG = 16
OWN_WORDS = 4
SWEEP_TARGET_WAVES, SWEEP_TARGET_WAVES_DENSE = 4096, 16384
SWEEP_CHUNK_BYTES = 1 << 20
SWEEP_MAX_PARTIAL_BYTES = 16 << 30
SORT_MIN_READS = 4096
ARENA_CHUNKS = 16
WIN_SIZE, WIN_STRIDE = 2560, 1024
WIN_MIN_ENTRIES = 32
WALK16_K = 16
MAX_READ_POS = (1 << 20) - 2           # include/wepp_place.h: 0xFFFFF is the padding event's position
W_PAD_POS = 0xFFFFF


# ---- plan arithmetic ------------------------------------------------------------------------------------------------
def tile_reads(maxk, T=64):
    """Reads per tile: T halves while T * maxk > MAX_TILE_ENTRIES."""
    while T > 1 and T * maxk > MAX_TILE_ENTRIES:
        T >>= 1
    return T


def takes_table(maxk, max_pos):
    """The dense (table) variant: reads of 16 words and more that fit LDS, on a tree whose positions stay below the
    reserved position field."""
    return DENSE_MIN_READ_WORDS <= maxk <= MAX_TILE_ENTRIES and max_pos < DENSE_MAX_POS


def tile_need(maxk, count, T=64):
    return min(min(tile_reads(maxk, T), count) * maxk, MAX_TILE_ENTRIES)


def ent_cap(maxk, count, T=64):
    """Read words of a tile in LDS, rounded to 64; 0 when a read is longer than LDS takes."""
    return (tile_need(maxk, count, T) + 63) & ~63 if maxk <= MAX_TILE_ENTRIES else 0


def key_cap(maxk, count, max_pos, T=64):
    """Sorted keys of a dense tile: a power of two, at least 64."""
    if not takes_table(maxk, max_pos):
        return 0
    k = 64
    while k < tile_need(maxk, count, T):
        k <<= 1
    return k


def chunks(ntiles, NB, ncp, cp_stride, sbytes, dense, count, win_tiles=None):
    """(nchunks, bpc) of a plan: chunks cut at checkpoints.  win_tiles: the tiles of all table window plans of the
    call, which share one launch."""
    n = max(1, ((SWEEP_TARGET_WAVES_DENSE if dense else SWEEP_TARGET_WAVES) + ntiles - 1) // ntiles)
    if win_tiles is not None:
        n = max(1, (SWEEP_TARGET_WAVES_DENSE + win_tiles - 1) // win_tiles)
    n = max(n, (sbytes + SWEEP_CHUNK_BYTES - 1) // SWEEP_CHUNK_BYTES)
    n = min(n, max(1, SWEEP_MAX_PARTIAL_BYTES // (count * 12)))
    n = min(n, max(1, NB // 8))
    if dense:
        n = max(n, DENSE_WAVES_PER_WG)
    n = min(n, ncp)
    bpc = (ncp + n - 1) // n * cp_stride
    nchunks = (NB + bpc - 1) // bpc
    if dense:
        nchunks = (nchunks + DENSE_WAVES_PER_WG - 1) // DENSE_WAVES_PER_WG * DENSE_WAVES_PER_WG
    return nchunks, bpc


def finalize_lanes_per_read(nchunks):
    return 1 if nchunks <= 8 else 4 if nchunks <= 32 else 16 if nchunks <= 128 else 64


def finalize_reads_per_workgroup(nchunks):
    return 256 // finalize_lanes_per_read(nchunks)


def stream_geometry(flat, stream=None):
    """NB, ncp, cp_stride and the bytes of one sweep of a stream of the flat image (default: the whole tree)."""
    n0 = flat.get("blk_node0", stream)
    NB = len(n0) - 1
    ncp = len(flat.get("cp_off", stream)) - 1
    if stream is None:
        return dict(NB=NB, ncp=ncp, cp_stride=int(flat.cp_stride), sbytes=int(flat.stats.stream_bytes))
    # (window streams and window crowns: <= 1024 checkpoints; an upper bound of the bytes, which the cases keep far
    # below one chunk's worth)
    E = len(flat.get("ev_word", stream))
    return dict(NB=NB, ncp=ncp, cp_stride=max(1, (NB + 1023) // 1024), sbytes=5 * E + 36 * NB)


def predict_plan(count, maxk, geom, max_pos, T=64, window=None, win_tiles=None):
    """What the `[plan]` line of a tile plan must say.  window = index of the genome window of a window plan."""
    Tp = tile_reads(maxk, T)
    ntiles = (count + Tp - 1) // Tp
    dense = takes_table(maxk, max_pos)
    table = dense and window is not None
    nchunks, bpc = chunks(ntiles, geom["NB"], geom["ncp"], geom["cp_stride"], geom["sbytes"], dense, count,
                          win_tiles if table else None)
    return dict(kind="window" if window is not None else "sweep", count=count, T=Tp, ntiles=ntiles, nchunks=nchunks,
                bpc=bpc, NB=geom["NB"], ncp=geom["ncp"], dense=int(dense), ent_cap=ent_cap(maxk, count, T),
                key_cap=window * WIN_STRIDE if table else key_cap(maxk, count, max_pos, T))


def parse_plan_line(line):
    """'[plan] sweep t=6 count=70 ...' -> dict(kind='sweep', t=6, count=70, ...)."""
    parts = line.split()
    assert parts[0] == "[plan]"
    d = dict(kind=parts[1])
    for kv in parts[2:]:
        k, v = kv.split("=")
        d[k] = int(v)
    return d


# ---- the input's side: trees, reads, tiles, events ------------------------------------------------------------------
class TreeInfo:
    """A tree with its flat image and what the builders ask about it."""

    def __init__(self, tree):
        self.tree = tree
        self.flat = w.FlatView(tree)
        self.max_pos = int(self.flat.stats.max_position)
        self.bm_words = 1
        while self.bm_words < (self.max_pos >> 5) + 1:
            self.bm_words <<= 1
        self.ref_at = {}
        for p, r in zip(tree.mut_pos.tolist(), tree.mut_ref.tolist()):
            if p >= 0:
                self.ref_at[p] = r
        self.mutated = sorted(self.ref_at)

    def ref(self, p):
        return self.ref_at.get(p, A)

    def muts(self, node):
        t = self.tree
        a, b = int(t.mut_off[node]), int(t.mut_off[node + 1])
        return [(int(t.mut_pos[i]), int(t.mut_ref[i]), int(t.mut_par[i]), int(t.mut_mut[i])) for i in range(a, b)]

    def genotype(self, node):
        """Entries (pos, ref, allele, 0) of a sample that carries exactly the alleles of `node`."""
        path = []
        while node >= 0:
            path.append(node)
            node = int(self.tree.parent[node])
        g = {}
        for n in reversed(path):
            for p, r, _, m in self.muts(n):
                if p >= 0:
                    g[p] = m
        return [(p, self.ref(p), a, 0) for p, a in sorted(g.items()) if a != self.ref(p)]

    def events(self, stream=None):
        """(positions of the stream's events, blk_eoff)."""
        return (self.flat.get("ev_word", stream) & 0xFFFFF).astype(np.int64), self.flat.get("blk_eoff", stream).astype(np.int64)

    def block_positions(self, b, stream=None):
        pos, eo = self.events(stream)
        return sorted(set(int(p) for p in pos[eo[b]:eo[b + 1]] if p != W_PAD_POS))

    def blocks_of(self, p, stream=None):
        pos, eo = self.events(stream)
        return sorted(set(int(np.searchsorted(eo, e, side="right")) - 1 for e in np.flatnonzero(pos == p)))


def read_lists(reads):
    out = []
    for r in range(reads.n_reads):
        p, rf, a, ms = reads.entries(r)
        out.append([(int(p[i]), int(rf[i]), int(a[i]), int(ms[i])) for i in range(len(p))])
    return out


def tiles_of(lists, T=64, sort=None):
    """Read indices of every tile of ONE plan that takes the whole batch, in list order (module docstring)."""
    n = len(lists)
    assert n <= 16384
    maxk = max([len(l) for l in lists] + [1])
    Tp = tile_reads(maxk, T)
    order = list(range(n))
    if n >= SORT_MIN_READS if sort is None else sort:
        order.sort(key=lambda r: lists[r][0][0] + 1 if lists[r] else 0)      # (stable, like the device's radix sort)
    return [order[i:i + Tp] for i in range(0, n, Tp)]


def tile_entries(lists, tile):
    """n_ent and n2 of a tile: its read words and the bitonic network's size."""
    n_ent = sum(len(lists[r]) for r in tile)
    n2 = 1
    while n2 < n_ent:
        n2 <<= 1
    return n_ent, n2


def tile_hits(info, lists, tile, stream=None):
    """Per block of the stream: (hit events among the block's first 128 event slots, events of the block).  A slot is
    a hit when its position's bit is set in the tile's bitmap: the positions <= max_pos its reads list, bit index
    masked by the map's size (the padding slots carry position 0xFFFFF)."""
    bits = set(p for r in tile for (p, _, _, _) in lists[r] if p <= info.max_pos)
    mask = 32 * info.bm_words - 1
    pos, eo = info.events(stream)
    is_hit = np.isin(pos & mask, np.fromiter(bits, np.int64, len(bits)))
    pad_hit = (W_PAD_POS & mask) in bits
    out = []
    for b in range(len(eo) - 1):
        e0, e1 = int(eo[b]), int(eo[b + 1])
        hits = int(is_hit[e0:min(e1, e0 + 128)].sum()) + (max(0, 128 - (e1 - e0)) if pad_hit else 0)
        out.append((hits, e1 - e0))
    return out


class Case:
    """tree, reads, knobs and facts of one case.  counts: the prefixes of the batch to place (default: all of it).
    window: the genome window whose plan takes every read of the batch (work skipping on), else the batch is one plan
    on the whole-tree stream (work skipping off)."""

    def __init__(self, name, tree, reads, walk=False, crowns=False, tile=64, facts=None, info=None, window=None):
        self.name, self.tree, self.reads = name, tree, reads
        self.knobs = dict(walk=walk, crowns=crowns, seeds=False, tile=tile)
        self.facts = facts or {}
        self.info = info or TreeInfo(tree)
        self.counts = (reads.n_reads,)
        self.window = window
        self.arena = None          # (window, crown): every read sweeps that window crown on its own (k_sweep_arena)
        assert crowns or window is None

    def lists(self):
        return read_lists(self.reads)

    def plan(self, count=None):
        """The one tile plan of the call that places the first `count` reads."""
        count = self.reads.n_reads if count is None else count
        k = np.diff(self.reads.read_off.astype(np.int64))[:count]
        stream = None if self.window is None else "w%d" % self.window
        Tp = tile_reads(int(max(1, k.max())), self.knobs["tile"])
        return predict_plan(count, int(max(1, k.max())), stream_geometry(self.info.flat, stream), self.info.max_pos,
                            self.knobs["tile"], window=self.window, win_tiles=(count + Tp - 1) // Tp)


def apply_knobs(mat, knobs):
    mat.set_use_walk(knobs["walk"])
    mat.set_use_crowns(knobs["crowns"])
    mat.set_use_seeds(knobs["seeds"])
    mat.set_tile_reads(knobs["tile"])


@functools.lru_cache(maxsize=None)
def base(n_nodes=2000, genome=2000, seed=7):
    """The common small tree: ~32 blocks of 64 nodes, nearly every position of its genome mutated somewhere."""
    g = w.generate_tree(seed, n_nodes, genome_len=genome, p_ambiguous=0.01, p_masked_node=0.002, root_mutations=2,
                        p_back_mutation=0.05)
    return TreeInfo(g.tree)


def _fill_word(info, p, rng):
    """A word at a position the read does not owe to its node: the reference allele, another one, or N."""
    u = rng.random()
    rf = info.ref(p)
    if u < 0.4:
        return (p, rf, rf, 0)
    if u < 0.8:
        return (p, rf, int(1 << rng.integers(0, 4)), 0)
    return (p, rf, N, 1)


def node_read(info, node, k, rng, pool, keep=()):
    """A read of exactly k words: the alleles of `node` (as many as fit; the positions in `keep` first), filled up with
    words at positions drawn from `pool`."""
    ents = {e[0]: e for e in info.genotype(node)}
    chosen = {p: ents[p] for p in keep if p in ents}
    for p in keep:
        if p not in chosen:
            chosen[p] = _fill_word(info, p, rng)
    rest = [p for p in ents if p not in chosen]
    rng.shuffle(rest)
    for p in rest[:max(0, k - len(chosen))]:
        chosen[p] = ents[p]
    pool = [p for p in pool if p not in chosen]
    assert len(chosen) + len(pool) >= k, "not enough positions for a read of %d words" % k
    for p in rng.choice(pool, size=k - len(chosen), replace=False).tolist() if len(chosen) < k else []:
        chosen[int(p)] = _fill_word(info, int(p), rng)
    assert len(chosen) == k
    return [chosen[p] for p in sorted(chosen)]


def node_batch(info, ks, seed, keep=(), pool=None):
    """One read per entry of ks, each following a random node of the tree."""
    rng = np.random.default_rng(seed)
    pool = list(range(1, info.max_pos + 1)) if pool is None else pool
    return [node_read(info, int(rng.integers(0, info.tree.n_nodes)), int(k), rng, pool, keep) for k in ks]


CASES = {}


def case(fn):
    CASES[fn.__name__] = functools.lru_cache(maxsize=None)(fn)
    return CASES[fn.__name__]


# ---- tile rule ------------------------------------------------------------------------------------------------------
def _tile_rule(name, ks, tile=64, seed=1, info=None, pool=None):
    info = info or base()
    lists = node_batch(info, ks, seed, pool=pool)
    facts = dict(count=len(ks), maxk=max(ks), n_ent=[tile_entries(lists, t) for t in tiles_of(lists, tile)])
    return Case(name, info.tree, Reads.from_lists(lists), tile=tile, facts=facts, info=info)


@case
def maxk_15():
    """70 reads, the longest of 15 words: the plain variant; the second tile holds 6 reads."""
    return _tile_rule("maxk_15", [15] + [int(k) for k in np.random.default_rng(15).integers(1, 16, 69)])


@case
def maxk_16():
    """The same batch with one word more in its longest read: the dense variant."""
    return _tile_rule("maxk_16", [16] + [int(k) for k in np.random.default_rng(15).integers(1, 16, 69)])


@case
def maxk_128():
    """64 reads of exactly 128 words: T = 64, n_ent = n2 = 8192, key index 8191 in use."""
    return _tile_rule("maxk_128", [128] * 64, seed=2)


@case
def maxk_129():
    """One read of 129 words among 64: T = 32."""
    return _tile_rule("maxk_129", [128] * 63 + [129], seed=2)


def _far_pool(info):
    # positions for reads longer than the genome: every third position up to 40 000 (beyond max_pos: listed, never hit)
    return list(range(1, info.max_pos + 1)) + list(range(info.max_pos + 3, 40000, 3))


@case
def maxk_8192():
    """A read of 8192 words between two short ones: T = 1, its words in LDS, n_ent = n2 = 8192."""
    return _tile_rule("maxk_8192", [20, 8192, 7], seed=3, pool=_far_pool(base()))


@case
def maxk_8193():
    """One word more: the read is swept alone with its words in global memory."""
    return _tile_rule("maxk_8193", [20, 8193, 7], seed=3, pool=_far_pool(base()))


for _n in (1, 64, 65):
    for _k, _kind in ((5, "plain"), (18, "dense")):
        def _count_case(n=_n, k=_k, kind=_kind):
            return _tile_rule("count_%d_%s" % (n, kind), [k] * n, seed=40 + n + k)
        _count_case.__name__ = "count_%d_%s" % (_n, _kind)
        _count_case.__doc__ = "%d reads of %d words (%s variant): tiles of 1, 64 and 64 + 1 reads." % (_n, _k, _kind)
        case(_count_case)

for _t in (1, 16, 64):
    for _k, _kind in ((5, "plain"), (18, "dense")):
        def _tile_case(t=_t, k=_k, kind=_kind):
            return _tile_rule("tile_%d_%s" % (t, kind), [k] * 70, tile=t, seed=50 + k)
        _tile_case.__name__ = "tile_%d_%s" % (_t, _kind)
        _tile_case.__doc__ = "70 reads of %d words with the tile knob at %d." % (_k, _t)
        case(_tile_case)


# ---- plain variant: OWN_WORDS words in registers, the rest in LDS; equal reads of <= OWN_WORDS words share a sweep ----
def _own_reads(info, n):
    """n pairs (read of 4 words, read of 5 words).  A read of 5 words is the genotype of a node that differs from the
    reference at exactly five positions (it is placed on that node with score 0); its partner is the same read without
    the fifth word -- the one word the plain sweep keeps in LDS only -- which is placed elsewhere.  The pairs cycle
    through the nodes of that kind."""
    nodes = [x for x in range(info.tree.n_nodes) if len(info.genotype(x)) == OWN_WORDS + 1]
    assert len(nodes) >= 20
    five = [info.genotype(nodes[i % len(nodes)]) for i in range(n)]
    return [f[:OWN_WORDS] for f in five], five


def _own_case(name, lists, tile, pairs):
    info = base()
    k = [len(l) for l in lists]
    tiles = tiles_of(lists, tile)
    where = {r: i for i, tl in enumerate(tiles) for r in tl}
    facts = dict(k=k, tiles=[[k[r] for r in tl] for tl in tiles],
                 pairs=[(a, b, where[a] == where[b], lists[a] == lists[b]) for a, b in pairs])
    return Case(name, info.tree, Reads.from_lists(lists), tile=tile, facts=facts, info=info)


@case
def own_4_and_5_one_tile():
    """Reads of 4 and of 5 words interleaved in one tile: tile_long is set, the short reads never search."""
    four, five = _own_reads(base(), 27)
    lists = [x for pair in zip(four, five) for x in pair]
    return _own_case("own_4_and_5_one_tile", lists, 64, [])


@case
def own_4_and_5_separate_tiles():
    """The same reads, the 4-word ones first, in tiles of 16: tiles without a long read, tiles of long reads only and
    one tile (the third) that holds both."""
    four, five = _own_reads(base(), 27)
    return _own_case("own_4_and_5_separate_tiles", four + five, 16, [])


@case
def own_identical_reads():
    """Word-for-word identical reads of 4 words (evaluated once per tile: grp) and of 5 words (no grouping) side by
    side in the first tile and again in the second; 130 reads, T = 64."""
    four, five = _own_reads(base(), 33)
    lists = []
    for i in range(32):
        lists += [four[i], five[i]]
    # slots 0..3: two equal reads of 4 words, two equal reads of 5 words, side by side
    lists[0:4] = [four[32], four[32], five[32], five[32]]
    lists += [four[32], five[32]] + lists[4:64] + [four[32], five[32], four[32], five[32]]
    assert len(lists) == 130
    pairs = [(0, 1), (2, 3), (0, 64), (2, 65), (126, 128), (127, 129), (0, 126)]
    return _own_case("own_identical_reads", lists, 64, pairs)


# ---- dense keys -----------------------------------------------------------------------------------------------------
def hit_facts(info, lists, tile=64, stream=None):
    """Per tile of the batch: blocks of the stream with 1-2 hit events, with DENSE_MIN_HITS or more, and with more than
    128 events."""
    out = []
    for tl in tiles_of(lists, tile):
        h = tile_hits(info, lists, tl, stream)
        out.append(dict(few=sum(1 for x, _ in h if 1 <= x < DENSE_MIN_HITS), many=sum(1 for x, _ in h if x >= DENSE_MIN_HITS),
                        over128=sum(1 for _, e in h if e > 128)))
    return out


def _block_with_positions(info, n, start=0, above=0):
    """The first block from `start` on that holds events of at least n distinct positions above `above`, and those."""
    NB = len(info.flat.get("blk_node0")) - 1
    for b in range(start, NB):
        ps = [p for p in info.block_positions(b) if p > above]
        if len(ps) >= n:
            return b, ps
    raise AssertionError("no block with %d positions" % n)


def _single_event_positions(info):
    """Positions with exactly one event in the whole-tree stream (mutated once, at a leaf), by block."""
    pos, eo = info.events()
    real = pos[pos != W_PAD_POS]
    vals, cnt = np.unique(real, return_counts=True)
    single = set(vals[cnt == 1].tolist())
    by_block = {}
    for b in range(len(eo) - 1):
        by_block[b] = sorted(set(int(p) for p in pos[eo[b]:min(eo[b + 1], eo[b] + 128)] if int(p) in single))
    return by_block


@case
def dense_run_of_64():
    """All 64 reads of a tile list one mutated position q: a run of 64 equal keys, walked by the lane of q's event
    (its block holds at least three more listed positions)."""
    info = base()
    b, ps = _block_with_positions(info, 4, start=5)
    keep = tuple(ps[:4])
    lists = node_batch(info, [18] * 64, 71, keep=keep)
    facts = dict(q=keep[0], block=b, listing_q=sum(1 for l in lists if any(e[0] == keep[0] for e in l)),
                 hits_in_block=tile_hits(info, lists, list(range(64)))[b][0], n_ent=tile_entries(lists, range(64)))
    return Case("dense_run_of_64", info.tree, Reads.from_lists(lists), facts=facts, info=info)


@case
def dense_window():
    """A tile that spans more than DENSE_WINDOW positions from its smallest one, plo: tree events at plo + 4095 (the
    last entry of the direct index), at plo + 4096 (the first position found by binary search) and far beyond, each in
    a block with three hit events or more."""
    info = base(2000, 29903)
    mutated = info.mutated
    for a in mutated:
        if a > DENSE_WINDOW and a + 1 in info.ref_at and (a - (DENSE_WINDOW - 1)) not in info.ref_at:
            break
    else:
        raise AssertionError("no two adjacent mutated positions")
    plo, bpos = a - (DENSE_WINDOW - 1), a + 1
    far = max(p for p in mutated if len(info.blocks_of(p)) > 0)
    keep = [plo, a, bpos, far]
    for x in (a, bpos, far):
        bx = info.blocks_of(x)[0]
        keep += [p for p in info.block_positions(bx) if p > plo and p not in keep][:2]
    lists = node_batch(info, [24] * 8, 72, keep=tuple(keep), pool=list(range(plo + 1, info.max_pos + 1)))
    tl = list(range(8))
    h = tile_hits(info, lists, tl)
    facts = dict(plo=min(e[0] for l in lists for e in l), at_4095=a, at_4096=bpos, far=far,
                 hits={x: max(h[b][0] for b in info.blocks_of(x)) for x in (a, bpos, far)},
                 listed={x: sum(1 for l in lists if any(e[0] == x for e in l)) for x in (plo, a, bpos, far)})
    return Case("dense_window", info.tree, Reads.from_lists(lists), facts=facts, info=info)


@case
def dense_n_ent_1024():
    """64 reads of 16 words: n_ent = n2 = 1024, no padding key."""
    return _tile_rule("dense_n_ent_1024", [16] * 64, seed=73)


@case
def dense_n_ent_1025():
    """One word more: n_ent = 1025, n2 = 2048, 1023 padding keys."""
    return _tile_rule("dense_n_ent_1025", [16] * 63 + [17], seed=73)


@case
def dense_hits_2_and_3():
    """Three reads of 16 words that list the same positions: two that have their only event in one block (lane = read
    loop, below DENSE_MIN_HITS), three that have theirs in another (lane = event lookup), the rest beyond max_pos."""
    info = base()
    by_block = _single_event_positions(info)
    b2 = next(b for b in sorted(by_block) if len(by_block[b]) >= 2)
    b3 = next(b for b in sorted(by_block) if len(by_block[b]) >= 3 and b != b2)
    ps = by_block[b2][:2] + by_block[b3][:3]
    t = info.tree
    allele = {int(t.mut_pos[i]): int(t.mut_mut[i]) for i in range(len(t.mut_pos)) if int(t.mut_pos[i]) in ps}
    rng = np.random.default_rng(74)
    far = [info.max_pos + 10 * (i + 1) for i in range(11)]
    lists = []
    for r in range(3):
        ents = [(p, info.ref(p), allele[p] if (r + i) % 2 == 0 else info.ref(p), 0) for i, p in enumerate(ps)]
        ents += [_fill_word(info, p, rng) for p in far]
        lists.append(sorted(ents))
    h = tile_hits(info, lists, [0, 1, 2])
    facts = dict(b2=b2, b3=b3, hits_b2=h[b2][0], hits_b3=h[b3][0], hit_blocks=sum(1 for x, _ in h if x))
    return Case("dense_hits_2_and_3", info.tree, Reads.from_lists(lists), facts=facts, info=info)


# ---- positions ------------------------------------------------------------------------------------------------------
HIGH = 1 << 19


def _shallow_internal(info):
    """An internal node X, few mutations from the root, with q = the position of its last mutation (away from the
    reference allele), and three more positions of the first block that holds an event at q."""
    t = info.tree
    kids = np.bincount(t.parent[1:], minlength=t.n_nodes)
    for x in range(1, t.n_nodes):
        m = info.muts(x)
        if kids[x] >= 1 and m and m[-1][0] > 0 and m[-1][1] == m[-1][2] and len(info.genotype(x)) <= 4:
            q = m[-1][0]
            b = info.blocks_of(q)[0]
            others = [p for p in info.block_positions(b) if p != q]
            if len(others) >= 3:
                return x, q, m[-1][3], b, others[:3]
    raise AssertionError("no such node")


def _chunk_mates(info, bpc, max_words):
    """An internal node X with q = the position of its last mutation (away from the reference allele) and a descendant
    D in the NEXT block of the same chunk of bpc blocks: what the sweep adds to a read's running count at X's enter
    event it still carries when it reaches D.  Plus three more positions of X's block."""
    t = info.tree
    flat = info.flat
    n0 = flat.get("blk_node0")
    dfs2id = flat.get("dfs2id")
    dfs_of = np.zeros(t.n_nodes, np.int64)
    dfs_of[dfs2id] = np.arange(t.n_nodes)
    for d in range(1, t.n_nodes):
        x = int(dfs2id[d])
        m = info.muts(x)
        b = int(np.searchsorted(n0, d, side="right")) - 1
        if not m or m[-1][0] <= 0 or m[-1][1] != m[-1][2] or b % bpc == bpc - 1 or b + 1 >= len(n0) - 1:
            continue
        q = m[-1][0]
        if sum(1 for p in t.mut_pos.tolist() if p == q) != 1:
            continue                                            # (q mutated once in the tree: one enter event, at X)
        others = [p for p in info.block_positions(b) if p != q]
        for dd in range(int(n0[b + 1]), int(n0[b + 2])):
            y = int(dfs2id[dd])
            anc = y
            while anc > 0 and anc != x:
                anc = int(t.parent[anc])
            if anc == x and y != x and len(info.genotype(y)) <= max_words and len(others) >= 3:
                return x, q, m[-1][3], b, others[:3], y
    raise AssertionError("no such pair of nodes")


def _moved(lists, r, q):
    """Read r with its word at q + 2^19 moved to q (replacing what it lists there)."""
    out = [e for e in lists[r] if e[0] not in (q, q + HIGH)]
    hi = next(e for e in lists[r] if e[0] == q + HIGH)
    return sorted(out + [(q, hi[1], hi[2], hi[3])])


def _pos_case(name, k, build, no_q=False):
    """Six reads of k words around the special ones that `build` returns (lists, facts); no_q: none of the others
    lists q either."""
    info = base()
    if k >= DENSE_MIN_READ_WORDS:
        # (the dense plan of six reads on this tree: chunks of two blocks)
        bpc = predict_plan(6, k, stream_geometry(info.flat), info.max_pos)["bpc"]
        x0, q, alt, b, others, x = _chunk_mates(info, bpc, k - 5)
    else:
        x, q, alt, b, others = _shallow_internal(info)
        x0 = x
    rng = np.random.default_rng(80 + k)
    keep = tuple(others) if k >= DENSE_MIN_READ_WORDS else ()
    pool = list(range(1, info.max_pos + 1))
    special, facts = build(info, x, q, alt, keep, rng, pool, k)
    rest = []
    while len(rest) < 6 - len(special):
        node = int(rng.integers(0, info.tree.n_nodes))
        if not (no_q and any(e[0] == q for e in info.genotype(node))):
            rest.append(node_read(info, node, k, rng, [p for p in pool if p != q], keep))
    lists = rest[:2] + special + rest[2:]
    facts.update(q=q, block=b, x=x0, d=x, k=[len(l) for l in lists], hits_in_block=tile_hits(info, lists, list(range(len(lists))))[b][0],
                 special=list(range(2, 2 + len(special))))
    return Case(name, info.tree, Reads.from_lists(lists), facts=facts, info=info), lists


def _x_read(info, x, q, keep, rng, pool, k, at_q, extra):
    """The alleles of node x with the word at q replaced by `at_q` (None: not listed), the words `extra`, filled up to k."""
    ents = [e for e in info.genotype(x) if e[0] != q] + ([at_q] if at_q else []) + list(extra)
    have = set(e[0] for e in ents)
    for p in keep:
        if p not in have and len(ents) < k:
            ents.append(_fill_word(info, p, rng))
            have.add(p)
    free = [p for p in pool if p not in have and p != q]
    for p in rng.choice(free, size=k - len(ents), replace=False).tolist():
        ents.append(_fill_word(info, int(p), rng))
    assert len(ents) == k
    return sorted(ents)


for _k, _kind in ((5, "plain"), (18, "dense")):
    def _pos_a(k=_k, kind=_kind):
        def build(info, x, q, alt, keep, rng, pool, k):
            rf = info.ref(q)
            return [_x_read(info, x, q, keep, rng, pool, k, (q, rf, rf, 0), [(q + HIGH, rf, alt, 0)])], {}
        c, lists = _pos_case("pos_a_%s" % kind, k, build)
        c.facts["moved"] = {2: _moved(lists, 2, c.facts["q"])}
        return c
    _pos_a.__name__ = "pos_a_%s" % _kind
    _pos_a.__doc__ = "One read lists q (mutated in the tree, reference allele in the read) and q + 2^19 (the tree's allele at q)."
    case(_pos_a)

    def _pos_b(k=_k, kind=_kind):
        def build(info, x, q, alt, keep, rng, pool, k):
            rf = info.ref(q)
            return [_x_read(info, x, q, keep, rng, pool, k, (q, rf, rf, 0), []),
                    _x_read(info, x, q, keep, rng, pool, k, None, [(q + HIGH, rf, alt, 0)])], {}
        c, lists = _pos_case("pos_b_%s" % kind, k, build)
        c.facts["moved"] = {3: _moved(lists, 3, c.facts["q"])}
        return c
    _pos_b.__name__ = "pos_b_%s" % _kind
    _pos_b.__doc__ = "Read A lists q, read B of the same tile lists q + 2^19 and not q."
    case(_pos_b)

    def _pos_e(k=_k, kind=_kind):
        def build(info, x, q, alt, keep, rng, pool, k):
            return [_x_read(info, x, q, keep, rng, pool, k, (q, info.ref(q), alt, 0), [(MAX_READ_POS, C, G, 0)])], {}
        return _pos_case("pos_e_%s" % kind, k, build)[0]
    _pos_e.__name__ = "pos_e_%s" % _kind
    _pos_e.__doc__ = "A read that lists position 2^20 - 2, the largest one a read word can carry."
    case(_pos_e)

    def _pos_f(k=_k, kind=_kind):
        def build(info, x, q, alt, keep, rng, pool, k):
            twin = q + 32 * info.bm_words
            assert twin > info.max_pos and (twin >> 5) & (info.bm_words - 1) == q >> 5 and twin & 31 == q & 31
            return [_x_read(info, x, q, keep, rng, pool, k, None, [(twin, info.ref(q), alt, 0)])], dict(twin=twin)
        c, lists = _pos_case("pos_f_%s" % kind, k, build, no_q=True)
        c.facts["listing_q"] = sum(1 for l in lists if any(e[0] == c.facts["q"] for e in l))
        return c
    _pos_f.__name__ = "pos_f_%s" % _kind
    _pos_f.__doc__ = "A position beyond max_pos on the bitmap word and bit of the mutated position q, which no read lists."
    case(_pos_f)


@functools.lru_cache(maxsize=None)
def _tree_ending_at(last):
    """The common tree with one leaf's last mutation moved to position `last`, the tree's largest."""
    info = base()
    t = info.tree
    kids = np.bincount(t.parent[1:], minlength=t.n_nodes)
    times = {}
    for p in t.mut_pos.tolist():
        times[p] = times.get(p, 0) + 1
    leaf = next(x for x in range(t.n_nodes - 1, 0, -1)
                if kids[x] == 0 and info.muts(x) and info.muts(x)[-1][0] > 0 and info.muts(x)[-1][1] == info.muts(x)[-1][2]
                and times[info.muts(x)[-1][0]] == 1 and len(info.muts(x)) >= 2)
    pos = t.mut_pos.copy()
    pos[t.mut_off[leaf + 1] - 1] = last
    return TreeInfo(Tree(t.parent, t.mut_off, pos, t.mut_ref, t.mut_mut, t.mut_par)), leaf


def _last_pos_case(name, last, k):
    info, leaf = _tree_ending_at(last)
    rng = np.random.default_rng(90 + k)
    b = info.blocks_of(last)[0]
    keep = (last,) + tuple(p for p in info.block_positions(b) if p != last)[:3]
    pool = list(range(1, 2001))
    lists = [node_read(info, int(rng.integers(0, info.tree.n_nodes)), k, rng, pool, keep if i % 2 else ()) for i in range(5)]
    lists.insert(2, node_read(info, leaf, k, rng, pool, keep))
    tl = list(range(6))
    facts = dict(max_pos=info.max_pos, last=last, block=b, hits_in_block=tile_hits(info, lists, tl)[b][0],
                 n_ent=tile_entries(lists, tl), listing_last=[r for r, l in enumerate(lists) if any(e[0] == last for e in l)],
                 leaf_word=next(e for e in lists[2] if e[0] == last))
    return Case(name, info.tree, Reads.from_lists(lists), facts=facts, info=info)


for _k, _kind in ((5, "plain"), (18, "long")):
    for _tag, _last in (("c_below", DENSE_MAX_POS - 1), ("c", DENSE_MAX_POS), ("d", DENSE_MAX_POS + 1)):
        def _pos_last(k=_k, kind=_kind, tag=_tag, last=_last):
            return _last_pos_case("pos_%s_%s" % (tag, kind), last, k)
        _pos_last.__name__ = "pos_%s_%s" % (_tag, _kind)
        _pos_last.__doc__ = ("A tree whose last mutated position is %d (2^19 %+d), listed by reads of a tile whose n_ent is no power of two."
                             % (_last, _last - HIGH))
        case(_pos_last)


# ---- blocks and chunks ----------------------------------------------------------------------------------------------
def _grown(n_nodes):
    """The generator of base() at another size (its block count follows the node count)."""
    return base(n_nodes, 2000)


HEAVY_MUTS = 150


@functools.lru_cache(maxsize=None)
def _heavy_tree():
    """The common tree with three nodes more: X, an internal node with HEAVY_MUTS mutations at positions of its own
    (2001 ...: a one-node block of more than 128 enter events, and as many exit events in front of the node that
    follows X's subtree), and two leaves below it."""
    info = base()
    t = info.tree
    n = t.n_nodes
    first = info.max_pos + 1
    xm = [(first + i, A, A, C) for i in range(HEAVY_MUTS)]
    muts = [info.muts(i) if t.mut_off[i + 1] > t.mut_off[i] else [] for i in range(n)]
    # (masked mutations keep their position -1)
    parent = t.parent.tolist() + [1, n, n]
    muts += [xm, [(first + HEAVY_MUTS, A, A, G)], [(first + HEAVY_MUTS + 1, A, A, T)]]
    return TreeInfo(Tree.from_lists(parent, muts)), n


def _overflow(info, stream=None):
    """Blocks of more than 128 events and the positions of their events from the 129th on."""
    pos, eo = info.events(stream)
    return {b: sorted(set(int(p) for p in pos[eo[b] + 128:eo[b + 1]] if p != W_PAD_POS))
            for b in range(len(eo) - 1) if eo[b + 1] - eo[b] > 128}


def _heavy_case(name, k, crowns=False, pool_lo=1):
    info, x = _heavy_tree()
    over = _overflow(info)
    keep = tuple(sorted(set(p for ps in over.values() for p in ps))[-3:])
    rng = np.random.default_rng(100 + k)
    pool = list(range(pool_lo, info.max_pos + 1))
    nodes = [x, x + 1, x + 2, 1] + [int(v) for v in rng.integers(0, info.tree.n_nodes, 6)]
    lists = [node_read(info, nd, k, rng, pool, keep if i < 6 else ()) for i, nd in enumerate(nodes)]
    if pool_lo > 1:
        lists = [[e for e in l if e[0] >= pool_lo] for l in lists]
        lists = [l + [_fill_word(info, int(p), rng) for p in rng.choice([p for p in pool if p not in set(e[0] for e in l)], size=k - len(l), replace=False)] for l in lists]
        lists = [sorted(l) for l in lists]
    facts = dict(over=over, keep=keep, k=[len(l) for l in lists])
    return Case(name, info.tree, Reads.from_lists(lists), crowns=crowns, facts=facts, info=info, window=1 if crowns else None)


@case
def heavy_block_plain():
    """Reads of 5 words that list positions among the overflow events of a block of more than 128 events."""
    return _heavy_case("heavy_block_plain", 5)


@case
def heavy_block_dense():
    """The same with reads of 18 words: the dense variant's overflow loops."""
    return _heavy_case("heavy_block_dense", 18)


@case
def heavy_block_window():
    """The same with reads of 40 words inside genome window 1 (positions 1024 ..), work skipping on: the window table
    variant on the window's stream, which holds the heavy node too."""
    c = _heavy_case("heavy_block_window", 40, crowns=True, pool_lo=WIN_STRIDE)
    c.facts["over_w1"] = _overflow(c.info, "w1")
    return c


CHUNK_TREES = {59: 3698, 60: 3760, 61: 3822, 121: 7622}       # blocks of the whole-tree stream: nodes of the tree


def _chunk_case(nb):
    info = _grown(CHUNK_TREES[nb])
    rng = np.random.default_rng(nb)
    lists = node_batch(info, [int(k) for k in rng.integers(1, 7, 4100)], 200 + nb)
    return Case("chunk_%d" % nb, info.tree, Reads.from_lists(lists), tile=1, facts=dict(count=len(lists)), info=info)


for _nb in CHUNK_TREES:
    def _cc(nb=_nb):
        return _chunk_case(nb)
    _cc.__name__ = "chunk_%d" % _nb
    _cc.__doc__ = ("4100 short reads, one per tile: one chunk of %d blocks per tile -- groups of 60 blocks, four blocks in "
                   "flight --, the list sorted by first position." % _nb)
    case(_cc)


# ---- finalize -------------------------------------------------------------------------------------------------------
# nchunks of a plain plan of few tiles = NB / 8 chunks of 8 blocks: nodes of the tree by the chunks wanted
FINALIZE_TREES = {8: 4482, 9: 4544, 32: 16232, 33: 16728, 128: 65128, 129: 65616}
FINALIZE_COUNTS = {8: (3,), 9: (64, 65), 32: (7,), 33: (16, 17), 128: (2,), 129: (4, 5)}


def _finalize_case(nchunks):
    info = _grown(FINALIZE_TREES[nchunks])
    counts = FINALIZE_COUNTS[nchunks]
    rng = np.random.default_rng(nchunks)
    lists = node_batch(info, [int(k) for k in rng.integers(1, 16, max(counts))], 300 + nchunks)
    c = Case("finalize_%d" % nchunks, info.tree, Reads.from_lists(lists), facts=dict(nchunks=nchunks), info=info)
    c.counts = counts
    return c


for _nc in FINALIZE_TREES:
    def _fc(nc=_nc):
        return _finalize_case(nc)
    _fc.__name__ = "finalize_%d" % _nc
    _fc.__doc__ = ("A tree whose whole-tree stream is cut into %d chunks, batches of %s reads: %d lanes per read, %d reads per workgroup."
                   % (_nc, " and ".join(str(x) for x in FINALIZE_COUNTS[_nc]), finalize_lanes_per_read(_nc), finalize_reads_per_workgroup(_nc)))
    case(_fc)


@case
def finalize_one_chunk():
    """A tree whose root has one child B, with two mutations, above 5 000 nodes: reads that list B's two positions with
    the reference allele score at least 2 more below B than at the root, so only the first chunk (the root's) holds a
    node within the bound root score + 1 and every other partial carries count 0."""
    rng = np.random.default_rng(7)
    n = 5000
    parent = [-1, 0] + [int(rng.integers(1, i)) for i in range(2, n)]
    muts = [[], [(5, A, A, C), (9, G, G, T)]] + [[(int(rng.integers(20, 1500)), A, A, int(rng.choice([C, G, T])))] for _ in range(2, n)]
    info = TreeInfo(Tree.from_lists(parent, muts))
    lists = []
    for r in range(9):
        extra = sorted(set(int(p) for p in rng.integers(1500, 1900, r % 4)))
        lists.append([(5, A, A, 0), (9, G, G, 0)] + [(p, A, C, 0) for p in extra])
    return Case("finalize_one_chunk", info.tree, Reads.from_lists(lists), facts={}, info=info)


# ---- what the device must report ------------------------------------------------------------------------------------
PLAN_FIELDS = ("kind", "count", "T", "ntiles", "nchunks", "bpc", "NB", "ncp", "dense", "ent_cap", "key_cap")


def check_device_plans(case, count, rec, plans, ctx=""):
    """The per-read plan classes (Mat.last_plans) and the `[plan]` lines of the call that placed the first `count`
    reads of `case` against the restated rule."""
    pcls = np.asarray(rec["pcls"])
    if case.arena is not None:
        # (one wave per read and chunk of its crown: no tile plan, no `[plan]` line; Mat.last_crowns names the crown
        # of the reads that walked only -- which crown a sweeping read takes is window_crown_of()'s restatement)
        assert (pcls == w.PLAN_SWEEP).all() and (np.asarray(rec["pst"]) == w.WINDOW_CROWN_SLOT).all(), (ctx, rec["pcls"], rec["pst"])
        assert plans == [], (ctx, plans)
        return
    if case.window is not None:
        assert (pcls == w.PLAN_WIN).all() and (np.asarray(rec["pst"]) == case.window).all(), (ctx, rec["pcls"], rec["pst"])
    else:
        assert (pcls == w.PLAN_SWEEP).all(), (ctx, rec["pcls"])
        assert (np.asarray(rec["pst"]) == case.info.flat.n_streams - 1).all(), (ctx, rec["pst"])
    want = case.plan(count)
    assert len(plans) == 1, (ctx, plans)
    assert {k: plans[0][k] for k in PLAN_FIELDS} == want, (ctx, plans[0], want)


# ---- window table variant -------------------------------------------------------------------------------------------
# Work skipping on, walks off: a read of more than WIN_MIN_ENTRIES words whose positions all lie in the genome window
# of its first one (WIN_SIZE positions from a multiple of WIN_STRIDE) joins that window's plan -- on these small
# trees, where no crown is smaller, the whole tree as the window sees it --, with the table variant of the sweep.
def _window_reads(info, ks, seed, window, keep=(), hi=None):
    lo = window * WIN_STRIDE
    hi = min(lo + WIN_SIZE - 1, info.max_pos) if hi is None else hi
    pool = list(range(max(lo, 1), hi + 1))
    rng = np.random.default_rng(seed)
    lists = []
    for k in ks:
        node = int(rng.integers(0, info.tree.n_nodes))
        l = [e for e in node_read(info, node, min(k, len(pool)), rng, pool, keep) if lo <= e[0] <= hi or e[0] in keep]
        free = [p for p in pool if p not in set(e[0] for e in l)]
        l += [_fill_word(info, int(p), rng) for p in rng.choice(free, size=k - len(l), replace=False)]
        lists.append(sorted(l))
    return lists


@case
def win_64_65_words():
    """Reads of exactly 64 words (all of them in the staging register) and of 65 (the last word read again) in a
    window plan."""
    info = base()
    lists = _window_reads(info, [64, 65, 64, 65, 40, 33, 65], 401, 0)
    return Case("win_64_65_words", info.tree, Reads.from_lists(lists), crowns=True, window=0, facts=dict(k=[len(l) for l in lists]), info=info)


@case
def win_tiles():
    """Tiles of 31, 32, 33 and 64 reads: the read masks are filled in 32-bit halves."""
    info = base()
    lists = _window_reads(info, [34 + i % 5 for i in range(64)], 402, 1)
    c = Case("win_tiles", info.tree, Reads.from_lists(lists), crowns=True, window=1, info=info)
    c.counts = (31, 32, 33, 64)
    return c


def _window_edge_tree(last):
    info, leaf = _tree_ending_at(last)
    assert WIN_STRIDE in info.ref_at
    return info, leaf


@case
def win_first_and_last_position():
    """A tree whose last mutated position is the last one of genome window 1; reads that list the window's first and
    last position (table entries 0 and WIN_SIZE - 1), one of them the leaf that carries the last mutation."""
    info, leaf = _window_edge_tree(WIN_STRIDE + WIN_SIZE - 1)
    keep = (WIN_STRIDE, WIN_STRIDE + WIN_SIZE - 1)
    lists = _window_reads(info, [34] * 6, 403, 1, keep=keep, hi=2000)
    rng = np.random.default_rng(404)
    lf = [e for e in info.genotype(leaf) if e[0] >= WIN_STRIDE]
    have = set(e[0] for e in lf)
    lf += [_fill_word(info, p, rng) for p in ([WIN_STRIDE] if WIN_STRIDE not in have else [])]
    have = set(e[0] for e in lf)
    lf += [_fill_word(info, int(p), rng) for p in rng.choice([p for p in range(WIN_STRIDE + 1, 2000) if p not in have], size=34 - len(lf), replace=False)]
    lists.insert(3, sorted(lf))
    facts = dict(first=WIN_STRIDE, last=WIN_STRIDE + WIN_SIZE - 1, listing=[sum(1 for l in lists if any(e[0] == p for e in l)) for p in keep],
                 leaf_word=next(e for e in lists[3] if e[0] == keep[1]))
    return Case("win_first_and_last_position", info.tree, Reads.from_lists(lists), crowns=True, window=1, facts=facts, info=info)


@case
def win_just_outside():
    """The same with the last position one further: the reads no longer fit the window and take the whole tree."""
    info, leaf = _window_edge_tree(WIN_STRIDE + WIN_SIZE)
    keep = (WIN_STRIDE, WIN_STRIDE + WIN_SIZE)
    lists = _window_reads(info, [34] * 6, 403, 1, keep=keep, hi=2000)
    facts = dict(first=WIN_STRIDE, outside=WIN_STRIDE + WIN_SIZE, listing=[sum(1 for l in lists if any(e[0] == p for e in l)) for p in keep])
    return Case("win_just_outside", info.tree, Reads.from_lists(lists), crowns=True, window=None, facts=facts, info=info)


def pair_runs(info, lists, tile, stream, window):
    """Per block of a window stream: (pairs, lanes whose run of pairs crosses a multiple of 64).  A lane holds two
    events of the block's first 128; its run = one pair per read of the tile that lists either position."""
    lo = window * WIN_STRIDE
    n_at = {}
    for r in tile:
        for e in lists[r]:
            if lo <= e[0] < lo + WIN_SIZE:
                n_at[e[0]] = n_at.get(e[0], 0) + 1
    pos, eo = info.events(stream)
    out = []
    for b in range(len(eo) - 1):
        ev = [int(p) for p in pos[eo[b]:min(eo[b + 1], eo[b] + 128)]]
        ev += [W_PAD_POS] * (len(ev) % 2)
        start, crossing = 0, 0
        for l in range(len(ev) // 2):
            nn = n_at.get(ev[2 * l], 0) + n_at.get(ev[2 * l + 1], 0)
            if nn and start // 64 != (start + nn - 1) // 64:
                crossing += 1
            start += nn
        out.append((start, crossing))
    return out


@case
def win_pair_rounds():
    """64 reads that all list two positions whose events share a block of the window's stream: more than 64 (event,
    read) pairs in that block, so several pair rounds, with runs of pairs that begin in one round and end in the next
    (`carry`)."""
    info = base()
    pos, eo = info.events("w0")
    for b in range(2, len(eo) - 1):
        ps = sorted(set(int(p) for p in pos[eo[b]:min(eo[b + 1], eo[b] + 128)] if p != W_PAD_POS and p < WIN_SIZE))
        if len(ps) >= 2:
            break
    keep = (ps[0], ps[-1])
    lists = _window_reads(info, [33 + i % 3 for i in range(64)], 405, 0, keep=keep)
    runs = pair_runs(info, lists, list(range(64)), "w0", 0)
    facts = dict(block=b, keep=keep, listing=[sum(1 for l in lists if any(e[0] == p for e in l)) for p in keep],
                 pairs=runs[b][0], crossing=runs[b][1], blocks_over_64=sum(1 for n, _ in runs if n > 64))
    return Case("win_pair_rounds", info.tree, Reads.from_lists(lists), crowns=True, window=0, facts=facts, info=info)


# ---- k_sweep_arena: a read of 17 - 32 words inside a genome window sweeps its window crown in ARENA_CHUNKS chunks ----
WC_MAX = 7


def window_crown_of(info, l):
    """(window, crown) a read inside one genome window is sent to with work skipping on (k_route): the first crown of
    its window whose bound admits the read's root score, if it is smaller than the tree-wide stream of root score +
    words; None otherwise."""
    flat = info.flat
    ns = flat.n_streams
    th = sm.theta(flat, l)
    t = next((i for i in range(ns - 1) if th <= int(flat.stats.stream_tau[i])), ns - 1)
    wi = l[0][0] // WIN_STRIDE
    tau, nodes = flat.get("wc_tau").reshape(-1, WC_MAX), flat.get("wc_nodes").reshape(-1, WC_MAX)
    if l[-1][0] >= wi * WIN_STRIDE + WIN_SIZE or wi >= len(tau):
        return None
    for i in range(WC_MAX):
        if not nodes[wi, i]:
            break
        if th - len(l) <= int(tau[wi, i]):
            return (wi, i) if int(nodes[wi, i]) < int(flat.stats.stream_nodes[t]) else None
    return None


ARENA_CROWNS = {1: (9000, 2, 0), 15: (9000, 8, 3), 16: (12000, 8, 2), 17: (9000, 9, 3)}     # blocks: (nodes of the tree, window, crown)


@functools.lru_cache(maxsize=None)
def _arena_tree(n_nodes):
    g = w.generate_tree(11, n_nodes, p_ambiguous=0.01, p_masked_node=0.002, root_mutations=1)
    return TreeInfo(g.tree)


def _arena_case(nb):
    n_nodes, wi, ci = ARENA_CROWNS[nb]
    info = _arena_tree(n_nodes)
    tau = info.flat.get("wc_tau").reshape(-1, WC_MAX)[wi]
    root_base = int(info.flat.get("nkey")[0]) >> 32
    rs = int(tau[ci - 1]) + 1 if ci else int(tau[0])            # the smallest root score that crown ci takes
    lo = wi * WIN_STRIDE
    root_pos = set(p for p, _, _, _ in info.muts(0))
    stream = "c%d.%d" % (wi, ci)
    crown_pos = sorted(set(int(p) for p in info.events(stream)[0] if lo <= p < lo + WIN_SIZE and p not in root_pos))
    t = info.tree
    allele = {int(t.mut_pos[i]): int(t.mut_mut[i]) for i in range(len(t.mut_pos))}
    rng = np.random.default_rng(500 + nb)
    lists = []
    for k in (17, 32, 20, 25, 31, 18):
        alt = [int(p) for p in rng.choice(crown_pos, size=rs - root_base, replace=False)]
        rest = [int(p) for p in rng.choice([p for p in range(max(lo, 1), lo + WIN_SIZE) if p not in alt and p not in root_pos],
                                           size=k - len(alt), replace=False)]
        l = [(p, info.ref(p), allele[p], 0) for p in alt]
        l += [(p, info.ref(p), N, 1) if rng.random() < 0.3 else (p, info.ref(p), info.ref(p), 0) for p in rest]
        lists.append(sorted(l))
    geom = stream_geometry(info.flat, stream)
    bpc = (geom["ncp"] + ARENA_CHUNKS - 1) // ARENA_CHUNKS * geom["cp_stride"]
    facts = dict(crown=(wi, ci), NB=geom["NB"], bpc=bpc, chunks_used=(geom["NB"] + bpc - 1) // bpc, root_score=rs,
                 k=[len(l) for l in lists])
    c = Case("arena_%d" % nb, info.tree, Reads.from_lists(lists), crowns=True, facts=facts, info=info)
    c.arena = (wi, ci)
    return c


for _nb in ARENA_CROWNS:
    def _ac(nb=_nb):
        return _arena_case(nb)
    _ac.__name__ = "arena_%d" % _nb
    _ac.__doc__ = "Reads of 17 - 32 words whose window crown has %d block%s: cut into 16 chunks all the same." % (_nb, "" if _nb == 1 else "s")
    case(_ac)
