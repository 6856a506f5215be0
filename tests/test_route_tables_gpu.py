"""k_route with its tables built at upload (route_kernels.hip: k_route_tables), its one word per head slot
(route_pos.hpp, k_route_pos) and its reservations of a round in one round trip.

The tree has 30 000 nodes over 10 000 positions: ten genome windows with crowns and several tree-wide streams.  Reads
are built by construction from the tree's position table; the stream k_route gives a read, its events and its nesting
depths there are counted on the CPU (RouteModel of tests/test_step_groups.py over the flat image), and k_route's own
counters (WEPP_DEBUG_PLANS=1) are compared with that.  Results go into device arrays filled with 0x7FFFFFFF before every
call -- a read that lost its list slot keeps that value -- and are compared with the incremental checker."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import read_kinds as rk
import wepp_amd as w
from test_fused_step import NTHREADS, assert_checker, assert_equal, entry, position_table
from test_step_groups import RouteModel
from wepp_amd import Reads

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILL = 0x7FFFFFFF
WALK_LIMIT = 6                                   # device_mat.hpp: WALK_MAX_EVENTS
WALK8_K, WALK8_STACK, WALK16_K, WALK16_STACK = 8, 16, 16, 32
WALK16_TO_WAVE_MAX = 8
WAVE_MAX_EVENTS = 256
ROUTE_BLOCKS = 256
ENTRY_COUNTS = (0, 1, 2, 3, 8, 9, 16, 17)
ROUTE_LINE = re.compile(r"\[route\] reads=(\d+) resolved=(\d+) walk=(\d+),(\d+) wave=(\d+),(\d+) \(of them walkers of 9 - 16 entries: (\d+)\)")
SAT_LEN = 7                                      # a list of 7 events or more saturates a length field of 3 bits (the rtlen3 build)


def device_constants():
    """(WALK16_TO_WAVE_MAX, ROUTE_BLOCKS) of device_mat.hpp"""
    path = os.path.join(os.path.dirname(os.path.abspath(w.__file__)), "csrc", "device_mat.hpp")
    with open(path) as fh:
        text = fh.read()
    return (int(re.search(r"constexpr uint32_t WALK16_TO_WAVE_MAX = (\d+);", text).group(1)),
            int(re.search(r"#define WEPP_ROUTE_BLOCKS (\d+)", text).group(1)))


def make_tree():
    return w.generate_tree(61, 30000, genome_len=10000, p_ambiguous=0.02, p_masked_node=0.003, root_mutations=1)


class Router(RouteModel):
    """What k_route makes of a read of at most WALK16_K entries: resolved / walk8 / walk16 / small / big / other."""

    def __init__(self, fv):
        super().__init__(fv)
        self.nest = {}
        self.max_pos = int(fv.stats.max_position)

    def nests(self, stream):
        if stream not in self.nest:
            self.nest[stream] = self.fv.get("ix_nest", stream).astype(np.int64)
        return self.nest[stream]

    def lens(self, S, stream):
        off = self.list_offsets(stream)
        return [int(off[p + 1] - off[p] - 1) for (p, _, _, _) in S if p <= self.max_pos]

    def streams_of(self, S):
        """the tables k_route consults for the read, in its order: the window crown (if one serves it), the tree-wide stream"""
        t = self.tiers.route(S)
        first = self.stream_of(S) if S else t
        return [first] if first == t else [first, t]

    def route(self, S, consulted=None):
        """(what becomes of the read, its events in the last table consulted); consulted: a list that takes the tables"""
        k = len(S)
        if k > WALK16_K:
            return "other", 0
        ev = 0
        for stream in self.streams_of(S):
            if consulted is not None:
                consulted.append(stream)
            nest = self.nests(stream)
            ev = sum(self.lens(S, stream))
            op = sum(int(nest[p]) for (p, _, _, _) in S if p <= self.max_pos)
            if ev <= WALK_LIMIT:
                cls = "walk8" if k <= WALK8_K and op <= WALK8_STACK else "walk16" if op <= WALK16_STACK else None
            else:
                cls = None if op > WALK16_STACK else "many"
            if cls is not None:
                break
        if cls is None:
            return "other", ev
        if cls == "many":
            return ("small" if ev <= 64 else "big" if ev <= WAVE_MAX_EVENTS else "other"), ev
        return ("resolved" if ev == 0 else cls), ev

    def saturates(self, S):
        """a length field of 3 bits saturates in a table k_route consults for the read"""
        return any(n >= SAT_LEN for stream in self.streams_of(S) for n in self.lens(S, stream))


def kinds(tree, model, seed):
    """The reads of the per-read case, by construction: name -> list of samples."""
    counts, ref = position_table(tree)
    counts = np.concatenate([counts, np.zeros(max(0, model.max_pos + 2 - counts.size), counts.dtype)])
    ref = np.concatenate([ref, np.zeros(counts.size - ref.size, ref.dtype)])
    ref = np.where(ref == 0, 1 << (np.arange(ref.size) % 4), ref)
    rng = np.random.default_rng(seed)
    allp = np.arange(1, model.max_pos)
    hot, cold = allp[(counts[allp] >= 1) & (counts[allp] <= 3)], allp[counts[allp] == 0]
    stride, size = model.stride, model.size
    out = {}

    def sample(pos):
        return [entry(rng, p, ref) for p in np.sort(np.asarray(pos))]

    def in_window(k, n_hot, wi=None):
        wi = int(rng.integers(0, (model.max_pos - size) // stride + 1)) if wi is None else wi
        lo, hi = wi * stride, wi * stride + size
        h, c = hot[(hot >= lo) & (hot < hi)], cold[(cold >= lo) & (cold < hi)]
        return sample(np.concatenate([rng.choice(h, n_hot, replace=False), rng.choice(c, k - n_hot, replace=False)]))

    for k in ENTRY_COUNTS:
        out[f"k{k}"] = [in_window(k, int(rng.integers(0, min(k, 3) + 1))) if k else [] for _ in range(500)]
    # events only at the third or a later entry: two cold positions in front of one to three hot ones
    late = []
    while len(late) < 500:
        k = int(rng.integers(3, 9))
        c2 = np.sort(rng.choice(cold[cold < model.max_pos // 2], 2, replace=False))
        h = hot[(hot > c2[1]) & (hot < c2[0] + size)]
        if h.size >= k - 2:
            late.append(sample(np.concatenate([c2, rng.choice(h, k - 2, replace=False)])))
    out["late"] = late
    # the last head slots of a slice: an entry AT max_pos (its length reads head max_pos + 1) and one beyond it
    out["at_max"] = [sample(np.concatenate([rng.choice(hot[hot > model.max_pos - size], int(rng.integers(0, 3)), replace=False), [model.max_pos]])) for _ in range(300)]
    out["beyond"] = [sample(np.concatenate([rng.choice(hot[hot > model.max_pos - size], int(rng.integers(1, 3)), replace=False), [model.max_pos + 1]])) for _ in range(300)]
    # two windows: the first entry in window wi, the last one behind its end
    span = []
    while len(span) < 500:
        k = int(rng.integers(2, 9))
        a = int(rng.choice(hot[hot < model.max_pos - size - 1]))
        b = int(rng.choice(hot[hot >= (a // stride) * stride + size]))
        mid = allp[(allp > a) & (allp < b) & (counts[allp] <= 1)]
        span.append(sample(np.concatenate([[a, b], rng.choice(mid, k - 2, replace=False)])))
    out["span"] = span
    return out


def many_event_reads(tree, model, seed, n):
    """reads of 1 - 8 entries at the tree's most mutated positions: 7 events and more in their stream"""
    return rk.hot_position_reads(tree, np.random.default_rng(seed), n, hot=300, k_lo=1, k_hi=8)


def to_lists(reads):
    """the samples of a Reads batch as lists of (position, reference, alleles, missing)"""
    off = reads.read_off.astype(np.int64)
    ents = list(zip(*[x.tolist() for x in w.unpack_read_word(reads.read_word)]))
    return [ents[off[r]:off[r + 1]] for r in range(reads.n_reads)]


def place_filled(mat, reads):
    """wepp_place_batch_device into arrays pre-filled with FILL"""
    import torch
    dev = torch.device("cuda", 0)
    d_off = torch.from_numpy(reads.read_off.astype(np.int32)).to(dev)
    rw = reads.read_word if reads.read_word.size else np.zeros(1, np.uint32)
    d_word = torch.from_numpy(rw.astype(np.int32)).to(dev)
    outs = [torch.full((max(reads.n_reads, 1),), FILL, dtype=torch.int32, device=dev) for _ in range(4)]
    mat.place_batch_device(d_off.data_ptr(), d_word.data_ptr(), reads.n_reads, int(reads.read_off[-1]), *[o.data_ptr() for o in outs], 0)
    torch.cuda.synchronize()
    a = [o.cpu().numpy()[:reads.n_reads] for o in outs]
    return w.PlacementResult(a[0].view(np.uint32), a[1], a[2].view(np.uint32), a[3].view(np.uint32))


def route_counts(capfd):
    lines = ROUTE_LINE.findall(capfd.readouterr().err)
    assert lines, "no [route] line"
    v = [int(x) for x in lines[-1]]
    # (the walkers of 9 - 16 entries a block hands to the wave pass are counted with the reads of <= 64 events)
    return dict(reads=v[0], resolved=v[1], walk8=v[2], walk16=v[3] + v[6], small=v[4] - v[6], big=v[5], w16_to_wave=v[6])


def model_counts(classes):
    return {c: int(sum(1 for x in classes if x == c)) for c in ("resolved", "walk8", "walk16", "small", "big")}


@pytest.fixture(scope="module")
def world(oracle):
    g = make_tree()
    fv = w.FlatView(g.tree)
    model = Router(fv)
    by_kind = kinds(g.tree, model, 11)
    names = [n for n, v in by_kind.items() for _ in v]
    samples = [S for v in by_kind.values() for S in v]
    routed = [model.route(S) for S in samples]
    reads = Reads.from_lists(samples)
    many = many_event_reads(g.tree, model, 12, 3000)
    many_routed = [model.route(S) for S in to_lists(many)]
    inc = oracle.OracleTree(g.tree).incremental()
    yield dict(g=g, fv=fv, model=model, names=np.array(names), samples=samples, routed=routed, reads=reads, inc=inc,
               want=inc.place_batch(reads, nthreads=NTHREADS), many=many, many_routed=many_routed,
               want_many=inc.place_batch(many, nthreads=NTHREADS))
    fv.close()
    g.close()


def check_per_read_batch(world):
    model, names, samples, routed = world["model"], world["names"], world["samples"], world["routed"]
    assert 5500 <= len(samples) <= 7500, len(samples)
    assert world["fv"].n_streams >= 3, world["fv"].n_streams
    assert (model.wc_n[:(model.max_pos - model.size) // model.stride + 1, 0] > 0).all()       # every window has crowns
    cls = np.array([c for c, _ in routed])
    for k in ENTRY_COUNTS:
        assert (names == f"k{k}").sum() == 500
    assert set(cls[names == "k17"]) == {"other"} and set(cls[names == "k0"]) == {"resolved"}
    for c in ("resolved", "walk8", "walk16"):
        assert (cls == c).sum() >= 100, (c, model_counts(cls))
    # events at the third or a later entry only, and some there
    late = [S for S, n in zip(samples, names) if n == "late"]
    assert all(sum(model.lens(S[:2], st)) == 0 for S in late for st in model.streams_of(S))
    assert sum(1 for S, n, (c, ev) in zip(samples, names, routed) if n == "late" and ev > 0) >= 100      # (a crown need not hold a position's mutations)
    assert all(S[-1][0] == model.max_pos for S, n in zip(samples, names) if n == "at_max")
    assert all(S[-1][0] == model.max_pos + 1 for S, n in zip(samples, names) if n == "beyond")
    # reads inside a window served by a crown, and reads whose crown refuses them: two tables consulted
    crowned = [S for S in samples if S and len(S) <= WALK16_K and len(model.streams_of(S)) == 2]
    assert len(crowned) >= 2000, len(crowned)
    spans = [S for S, n in zip(samples, names) if n == "span"]
    assert all(S[-1][0] >= (S[0][0] // model.stride) * model.stride + model.size for S in spans)


def test_batches_hold_what_the_gpu_tests_are_about(world):
    """On the CPU: the per-read batch holds every kind, and the pools of the list test are large enough."""
    check_per_read_batch(world)
    pools = model_counts([c for c, _ in world["many_routed"]])
    assert pools["small"] >= 600 and pools["big"] >= 600, pools
    sat = np.array([world["model"].saturates(S) for S in to_lists(world["many"])])
    assert sat.sum() >= 500, int(sat.sum())


@pytest.mark.gpu
def test_per_read_paths(world, monkeypatch, capfd):
    """Every kind of the per-read batch against the checker, and k_route's counts against the model's."""
    check_per_read_batch(world)
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    mat = w.Mat(world["g"].tree)
    try:
        res = place_filled(mat, world["reads"])
        c = route_counts(capfd)
        assert_checker(res, world["want"], "per-read batch")
        want = model_counts([x for x, _ in world["routed"]])
        assert {k: c[k] for k in want} == want and c["reads"] == world["reads"].n_reads, (c, want)
        assert_equal(place_filled(mat, world["reads"]), res, "second call")
    finally:
        mat.close()


def block_batch(world, n_w16):
    """4 096 reads, sixteen per routing block, every block with two walkers of up to 8 entries, n_w16 of 9 - 16 entries,
    two reads of 7 - 64 events, two of more than 64 and a read k_route places itself (n_w16 = 9), or three of each
    but the last (n_w16 = 8)."""
    per = 4096 // ROUTE_BLOCKS
    cls = np.array([c for c, _ in world["routed"]])
    mcls = np.array([c for c, _ in world["many_routed"]])
    n = {"walk8": 2, "walk16": n_w16, "small": 2, "big": 2, "resolved": 1} if n_w16 == 9 else {"walk8": 3, "walk16": n_w16, "small": 3, "big": 2, "resolved": 0}
    assert sum(n.values()) == per
    both = rk.concat([world["reads"], world["many"]])
    want = np.concatenate([world["want"], world["want_many"]])
    pool = {c: np.flatnonzero(cls == c) for c in ("walk8", "walk16", "resolved")}
    pool.update({c: world["reads"].n_reads + np.flatnonzero(mcls == c) for c in ("small", "big")})
    idx = np.concatenate([np.concatenate([np.resize(np.roll(pool[c], -b * n[c]), n[c]) for c in n]) for b in range(ROUTE_BLOCKS)])
    assert idx.size == 4096
    return rk.take(both, idx), want[idx], {c: n[c] * ROUTE_BLOCKS for c in n}


@pytest.mark.gpu
@pytest.mark.parametrize("n_w16", [WALK16_TO_WAVE_MAX + 1, WALK16_TO_WAVE_MAX], ids=["own list", "to wave"])
def test_all_four_lists_in_one_block_and_round(world, monkeypatch, capfd, n_w16):
    """Every block reserves a range of all four lists in the same round: walkers of up to 8 entries, walkers of 9 - 16
    entries (a list of their own beyond WALK16_TO_WAVE_MAX of them in the block, the waves' list up to it), reads of
    7 - 64 events and reads of more."""
    assert device_constants() == (WALK16_TO_WAVE_MAX, ROUTE_BLOCKS)
    reads, want, n = block_batch(world, n_w16)
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    mat = w.Mat(world["g"].tree)
    try:
        res = place_filled(mat, reads)
        c = route_counts(capfd)
        assert_checker(res, want, f"{n_w16} walkers of 9 - 16 entries a block")
        assert {k: c[k] for k in n} == n, (c, n)
        assert c["w16_to_wave"] == (n["walk16"] if n_w16 == WALK16_TO_WAVE_MAX else 0), c
    finally:
        mat.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257])
def test_edges_of_the_grid(world, n):
    """Fewer reads than routing blocks, one block without a read, and the first count with two reads in a block."""
    idx = np.flatnonzero(np.array([c for c, _ in world["routed"]]) != "other")[::7][:n]
    assert idx.size == n
    mat = w.Mat(world["g"].tree)
    try:
        assert_checker(place_filled(mat, rk.take(world["reads"], idx)), world["want"][idx], f"{n} reads")
    finally:
        mat.close()


@pytest.mark.gpu
def test_two_rounds_per_block(world):
    """1 100 000 reads in one call -- 4 297 a routing block, more than the 4 096 of a round -- equal the two halves placed
    by a call each; the first 2 048 against the checker."""
    g = world["g"]
    reads = g.reads(31, 1_100_000, read_len=150, amplicon_len=400, amplicon_step=300, p_substitution=0.001, p_n=0.005)
    assert -(-reads.n_reads // ROUTE_BLOCKS) > 4 * 1024
    half = reads.n_reads // 2
    mat = w.Mat(g.tree)
    try:
        res = place_filled(mat, reads)
        a = place_filled(mat, rk.take(reads, np.arange(half)))
        b = place_filled(mat, rk.take(reads, np.arange(half, reads.n_reads)))
        for f in ("best_bfs_j", "score", "num_best", "flags"):
            assert (getattr(res, f) == np.concatenate([getattr(a, f), getattr(b, f)])).all(), f
        head = rk.take(reads, np.arange(2048))
        assert_checker(w.PlacementResult(*[getattr(res, f)[:2048] for f in ("best_bfs_j", "score", "num_best", "flags")]),
                       world["inc"].place_batch(head, nthreads=NTHREADS), "first 2 048 reads")
    finally:
        mat.close()


def make_tree_beyond_the_tables():
    """64 mutations on the root: every tree-wide bound is base(root) + 0 .. 27 >= 64, outside the theta table"""
    return w.generate_tree(62, 20000, genome_len=10000, p_ambiguous=0.02, p_masked_node=0.003, root_mutations=64)


def test_bounds_beyond_the_tables_exist():
    """On the CPU: the second tree's last bounded tree-wide stream has a bound of 64 or more (k_route: tab_ok == 0)."""
    g = make_tree_beyond_the_tables()
    fv = w.FlatView(g.tree)
    try:
        assert fv.n_streams >= 2 and int(fv.stats.stream_tau[fv.n_streams - 2]) >= 64, list(fv.stats.stream_tau)[:fv.n_streams]
    finally:
        fv.close()
        g.close()


@pytest.mark.gpu
def test_scans_where_the_tables_do_not_reach(oracle):
    """tab_ok == 0: the scans of the bounds stay in place; amplicon reads and reads at hot positions against the checker."""
    g = make_tree_beyond_the_tables()
    reads = rk.concat([g.reads(33, 3000, read_len=150, amplicon_len=400, amplicon_step=300, p_substitution=0.002, p_n=0.01),
                       rk.hot_position_reads(g.tree, np.random.default_rng(5), 1000, hot=300, k_lo=1, k_hi=8)])
    mat = w.Mat(g.tree)
    try:
        assert int(mat.stats.stream_tau[mat.stats.n_streams - 2]) >= 64
        assert_checker(place_filled(mat, reads), oracle.OracleTree(g.tree).incremental().place_batch(reads, nthreads=NTHREADS), "tab_ok == 0")
    finally:
        mat.close()
        g.close()


def make_nested_tree():
    """Long root paths full of back-mutations: positions whose lists nest ten deep and more, also inside the larger window
    crowns (on the first tree no position of a crown nests deeper than once)."""
    return w.generate_tree(61, 30000, genome_len=6000, zipf_s=1.2, p_back_mutation=0.6, depth_choices=16, p_ambiguous=0.02,
                           p_masked_node=0.003, root_mutations=1)


def refused_reads(tree, model, seed, n):
    """Reads of 16 entries inside one window, at its most mutated positions, that a window crown serves -- and refuses:
    the intervals they can hold open there outgrow a walk's stack, so k_route asks the tree-wide stream's table as
    well.  Picked by the model from 4 000 built ones."""
    counts, ref = position_table(tree)
    ref = np.where(ref == 0, 1 << (np.arange(ref.size) % 4), ref)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(4000):
        wi = int(rng.integers(0, (model.max_pos - model.size) // model.stride + 1))
        cand = np.arange(max(1, wi * model.stride), min(wi * model.stride + model.size, counts.size))
        top = cand[np.argsort(counts[cand], kind="stable")[::-1][:64]]
        S = [entry(rng, p, ref) for p in np.sort(rng.choice(top, WALK16_K, replace=False))]
        seen = []
        model.route(S, seen)
        if len(seen) == 2:
            out.append(S)
        if len(out) == n:
            break
    return out


@pytest.fixture(scope="module")
def nested(oracle):
    g = make_nested_tree()
    fv = w.FlatView(g.tree)
    samples = refused_reads(g.tree, Router(fv), 13, 300)
    reads = Reads.from_lists(samples) if samples else rk.empty_reads(0)
    want = oracle.OracleTree(g.tree).incremental().place_batch(reads, nthreads=NTHREADS) if samples else None
    yield dict(g=g, samples=samples, reads=reads, want=want)
    fv.close()
    g.close()


def test_reads_a_crown_refuses_exist(nested):
    """On the CPU: at least 100 reads for which k_route consults both tables."""
    assert len(nested["samples"]) >= 100, len(nested["samples"])


@pytest.mark.gpu
def test_crown_that_refuses_a_read(nested):
    """Reads inside a window whose crown refuses them (too deep a stack): the crown's table, then the tree-wide one."""
    assert len(nested["samples"]) >= 100
    mat = w.Mat(nested["g"].tree)
    try:
        assert_checker(place_filled(mat, nested["reads"]), nested["want"], "reads their window crown refuses")
    finally:
        mat.close()


def variant_lib(name, *flags):
    lib = os.path.join(ROOT, "variants", name, "libwepp_place.so")
    csrc = os.path.join(ROOT, "wepp_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".hpp")))
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        subprocess.run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), name, *flags], check=True, capture_output=True, timeout=1500)
    return lib


@pytest.mark.gpu
def test_saturated_length_fields(world):
    """The rtlen3 build (a length field of 3 bits) in a child process: reads with a list of 7 events or more at one of
    their positions -- picked by the model, at least 500 -- take the exact list heads, mixed with reads that do not;
    the four arrays equal the checker's and the default build's."""
    model = world["model"]
    sat = np.array([model.saturates(S) for S in to_lists(world["many"])])
    plain = np.array([not model.saturates(S) and len(S) <= WALK16_K and len(S) > 0 for S in world["samples"]])
    assert sat.sum() >= 500 and plain.sum() >= 500, (int(sat.sum()), int(plain.sum()))
    i_sat, i_plain = np.flatnonzero(sat)[:1500], np.flatnonzero(plain)[:1500]
    # interleaved, so that every wave of k_route holds both kinds
    n = min(i_sat.size, i_plain.size)
    both = rk.concat([world["many"], world["reads"]])
    idx = np.stack([i_sat[:n], world["many"].n_reads + i_plain[:n]], 1).reshape(-1)
    reads, want = rk.take(both, idx), np.concatenate([world["want_many"], world["want"]])[idx]
    mat = w.Mat(world["g"].tree)
    try:
        res = place_filled(mat, reads)
    finally:
        mat.close()
    assert_checker(res, want, "default build")
    lib = variant_lib("rtlen3", "-DWEPP_RT_LEN_BITS=3")
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), read_off=reads.read_off, read_word=reads.read_word)
        run = subprocess.run([sys.executable, os.path.join(HERE, "route_variant_child.py"), os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")],
                             env=dict(os.environ, WEPP_PLACE_LIB=lib), capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
        assert json.loads(run.stdout.strip().splitlines()[-1])["len_bits"] == 3
        out = np.load(os.path.join(tmp, "out.npz"))
        got = w.PlacementResult(out["best_bfs_j"], out["score"], out["num_best"], out["flags"])
    assert_checker(got, want, "length fields of 3 bits")
    assert_equal(got, res, "length fields of 3 bits against the default build")
