"""The plain walkers of k_step by lane groups (place_dev.hpp: group_read, walk_kernels.hip: group_body): G lanes a read,
one lane per event, G = 8 for the default walk limit and 16 for a limit of up to 16 events.

The tree has 8 000 nodes over 3 000 positions, most of them mutated 0 - 3 times, so a read of 1 - 8 entries -- some at
positions with 1 - 3 mutations, the rest at positions without any -- holds 1 - 17 events in the stream k_route gives it:
the batch covers every total a group of 8 takes (1 - 6 by default, up to 8), the totals at the limits (6 / 7, 8 / 9,
16 / 17) and every entry count.  A read's events are counted on the CPU in the stream k_route picks for it (the
tree-wide crown of sweep_model.TieredModel, or the window crown its root score admits when that is smaller), and the
walkers k_route reports are compared with that count.  The incremental checker is the reference, computed once."""
import os
import re

import numpy as np
import pytest

import read_kinds as rk
import sweep_model as sm
import wepp_amd as w
from test_fused_step import NTHREADS, ROUTE_LINE, assert_checker, assert_equal, entry, position_table
from wepp_amd import Reads

N_READS = 6000
SEED = 7
TOTALS = tuple(range(1, 10)) + (16, 17)
WALK_LIMIT, WALK_LIMIT_WIDE = 6, 16          # WALK_MAX_EVENTS, WALK_MAX_EVENTS_BY_JOBS of device_mat.hpp
WALK8_K = 8


def make_tree():
    return w.generate_tree(61, 8000, genome_len=3000, p_ambiguous=0.02, p_masked_node=0.003, root_mutations=1)


def make_samples(tree, n, seed, k_of=None, hot_of=None):
    """n reads of 1 - 8 entries at distinct positions: 1 .. k of them at positions with 1 - 3 mutations in the tree, the
    others at positions without (their reference allele is made up: the tree never says it)."""
    counts, ref = position_table(tree)
    rng = np.random.default_rng(seed)
    hot, cold = np.flatnonzero((counts >= 1) & (counts <= 3)), np.flatnonzero(counts == 0)
    ref = np.where(ref == 0, 1 << (np.arange(ref.size) % 4), ref)
    samples = []
    for _ in range(n):
        k = int(rng.integers(1, WALK8_K + 1)) if k_of is None else k_of
        n_hot = int(rng.integers(1, k + 1)) if hot_of is None else hot_of
        pos = np.sort(np.concatenate([rng.choice(hot, n_hot, replace=False), rng.choice(cold, k - n_hot, replace=False)]))
        samples.append([entry(rng, p, ref) for p in pos])
    return samples


class RouteModel:
    """The stream k_route gives a read (route_kernels.hip) and the read's events in it."""

    def __init__(self, fv):
        self.fv = fv
        self.tiers = sm.TieredModel(fv)
        self.stride, self.size = int(fv.stats.window_stride), int(fv.stats.window_size)
        self.wc_tau, self.wc_n = fv.get("wc_tau").reshape(-1, w.WINDOW_CROWN_LEVELS), fv.get("wc_nodes").reshape(-1, w.WINDOW_CROWN_LEVELS)
        self.off = {}

    def list_offsets(self, stream):
        if stream not in self.off:
            self.off[stream] = self.fv.get("ix_head", stream)[:, 0].astype(np.int64)
        return self.off[stream]

    def stream_of(self, S):
        t = self.tiers.route(S)
        stream = t
        wi = S[0][0] // self.stride
        if S[-1][0] < wi * self.stride + self.size and wi < len(self.wc_n):
            rs = sm.theta(self.fv, S) - len(S)
            for i in range(w.WINDOW_CROWN_LEVELS):
                if not self.wc_n[wi, i]:
                    break
                if rs <= self.wc_tau[wi, i]:
                    if self.wc_n[wi, i] < len(self.tiers.models[t].nkey):
                        stream = f"c{wi}.{i}"
                    break
        return stream

    def events_of(self, S):
        off = self.list_offsets(self.stream_of(S))
        return int(sum(off[p + 1] - off[p] - 1 for (p, _, _, _) in S if p + 1 < len(off)))


def sub(want, idx):
    """the checker's records (a structured array) of the reads `idx`"""
    return want[idx]


@pytest.fixture(scope="module")
def world(oracle):
    """The tree, the batch, every read's entry count and routed events, and the checker's results for the batch."""
    g = make_tree()
    fv = w.FlatView(g.tree)
    model = RouteModel(fv)
    samples = make_samples(g.tree, N_READS, SEED)
    events = np.array([model.events_of(S) for S in samples])
    ks = np.array([len(S) for S in samples])
    # all walkers of 8 entries and 6 events: reads with 8 entries, 3 - 6 of them at mutated positions, those that keep 6 events
    full = [S for hot in (3, 4, 5, 6) for S in make_samples(g.tree, 250, SEED + hot, k_of=WALK8_K, hot_of=hot)]
    full = [S for S in full if model.events_of(S) == WALK_LIMIT]
    reads, full_reads = Reads.from_lists(samples), Reads.from_lists(full)
    inc = oracle.OracleTree(g.tree).incremental()
    yield dict(g=g, reads=reads, events=events, ks=ks, model=model, inc=inc, want=inc.place_batch(reads, nthreads=NTHREADS),
               full=full_reads, want_full=inc.place_batch(full_reads, nthreads=NTHREADS))
    fv.close()
    g.close()


def check_coverage(events, ks):
    for t in TOTALS:
        assert (events == t).sum() >= 3, (t, np.bincount(events).tolist())
    for k in range(1, WALK8_K + 1):
        assert (ks == k).sum() >= 3, (k, np.bincount(ks).tolist())
    # 1 .. 8 events with every entry count that can carry them: a read of few entries has a low bound, is routed to a small
    # crown and keeps there about one event per entry, so e events come with min(e, 4) entries or more
    for e in range(1, 9):
        for k in range(min(e, 4), WALK8_K + 1):
            assert ((events == e) & (ks == k)).any(), (e, k)


def test_batch_covers_every_total_and_entry_count(world):
    """On the CPU: the batch holds what the GPU tests below are about."""
    check_coverage(world["events"], world["ks"])
    assert world["full"].n_reads >= 64, world["full"].n_reads


def handle(monkeypatch, tree, env):
    """A fresh handle with the switches `env` (they are read when the handle is created)."""
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return w.Mat(tree)


STEP_LINE = re.compile(r"\[step\] walkers by groups of (\d+) lanes \(0: lane = read\); plain walkers of the previous call: (\d+)")


def debug_lines(capfd):
    """What the last call of a WEPP_DEBUG_PLANS=1 handle printed: k_route's counters (reads, walk8, ...) and the form
    of k_step's walkers as (lanes of a group -- 0: lane = read --, plain walkers of the call before)."""
    err = capfd.readouterr().err
    route, step = ROUTE_LINE.findall(err), STEP_LINE.findall(err)
    assert route and step, err[-500:]
    v = [int(x) for x in route[-1]]
    return dict(reads=v[0], resolved=v[1], walk8=v[2], walk16=v[3], wave_small=v[4], wave_big=v[5]), (int(step[-1][0]), int(step[-1][1]))


def step_form(capfd):
    return debug_lines(capfd)[1]


GROUPS_OFF = {"WEPP_STEP_GROUPS": "0"}
UNFUSED = {"WEPP_STEP_UNFUSED": "1"}
BY_JOBS = {"WEPP_WW_BLOCK_MAX_SMALL": "0", "WEPP_WW_BLOCK_MAX_BIG": "0"}
WIDE = {"WEPP_WALK_MAX_EVENTS": str(WALK_LIMIT_WIDE)}          # plain walkers of up to 16 events: groups of 16 lanes


@pytest.mark.gpu
def test_batch_against_checker_and_other_forms(world, monkeypatch, capfd):
    """The batch on a fresh handle against the checker, twice; the same arrays with the groups off, from the three
    launches k_step replaced, from a handle by jobs and from groups of 16 lanes; and k_route's count of plain walkers
    against the model's, for both walk limits."""
    check_coverage(world["events"], world["ks"])
    tree = world["g"].tree
    reads, events, ks = world["reads"], world["events"], world["ks"]
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    mat = handle(monkeypatch, tree, {})
    try:
        res = mat.place_batch(reads)
        c, step = debug_lines(capfd)
        assert step == (8, 0), step
        assert_checker(res, world["want"], "groups of 8")
        assert_equal(mat.place_batch(reads), res, "groups of 8, second call")
        assert c["walk8"] == int(((events >= 1) & (events <= WALK_LIMIT) & (ks <= WALK8_K)).sum()), (c, np.bincount(events).tolist())
    finally:
        mat.close()
    for env, ctx in ((GROUPS_OFF, "lane = read"), (UNFUSED, "three launches"), (BY_JOBS, "by jobs"), (WIDE, "groups of 16")):
        m2 = handle(monkeypatch, tree, env)
        try:
            got = m2.place_batch(reads)
            c, step = debug_lines(capfd) if env is not UNFUSED else (None, None)
            assert_equal(got, res, ctx)
            if env is UNFUSED:          # (no k_step: three launches)
                continue
            assert step[0] == {id(GROUPS_OFF): 0, id(BY_JOBS): 8, id(WIDE): 16}[id(env)], (ctx, step)
            assert_equal(m2.place_batch(reads), res, f"{ctx}, second call")
            limit = WALK_LIMIT_WIDE if env is WIDE else WALK_LIMIT
            assert c["walk8"] == int(((events >= 1) & (events <= limit) & (ks <= WALK8_K)).sum()), (ctx, c)
        finally:
            m2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, WIDE], ids=["G8", "G16"])
def test_edge_batches(world, monkeypatch, capfd, env):
    """Batches at the edges of the group-role workgroups, each on a fresh handle against the checker: one walker, a wave
    full of groups and one group over, a count that is no multiple of the reads of a workgroup, 40 000 and 60 000
    walkers (the workgroups loop: the grid is a workgroup per 128 reads and the 2 560 of the wave role, which take the
    group role when no read asks for the wave role, and a workgroup takes 128 / G reads per pass -- a second pass from
    21 846 walkers on for G = 16 and from 46 812 on for G = 8), and walkers that all hold 8 entries and 6 events."""
    tree = world["g"].tree
    group = 16 if env is WIDE else 8
    limit = WALK_LIMIT_WIDE if env is WIDE else WALK_LIMIT
    per_wave, per_wg = 64 // group, 2 * (64 // group)
    walkers = np.flatnonzero((world["events"] >= 1) & (world["events"] <= limit))
    assert walkers.size > 3 * per_wg + 5
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    picks = {"one walker": walkers[:1], "a wave full": walkers[:per_wave], "one group over": walkers[:per_wave + 1],
             "no multiple of a workgroup": walkers[:3 * per_wg + 5], "40 000 walkers": np.resize(walkers, 40_000), "60 000 walkers": np.resize(walkers, 60_000)}
    batches = [(name, rk.take(world["reads"], idx), sub(world["want"], idx), idx.size) for name, idx in picks.items()]
    batches.append(("8 entries and 6 events", world["full"], world["want_full"], world["full"].n_reads))
    for name, reads, want, n_walk in batches:
        mat = handle(monkeypatch, tree, env)
        try:
            res = mat.place_batch(reads)
            c, step = debug_lines(capfd)
            assert step == (group, 0), (name, step)
            assert_checker(res, want, f"G={group}, {name}")
            assert c["walk8"] == n_walk and c["reads"] == reads.n_reads, (name, c)
        finally:
            mat.close()


def max_group_walkers():
    """STEP_GROUPS_MAX_WALKERS of device_mat.hpp: plain walkers of a call up to which the next call goes by groups."""
    path = os.path.join(os.path.dirname(os.path.abspath(w.__file__)), "csrc", "device_mat.hpp")
    with open(path) as fh:
        return int(re.search(r"constexpr uint32_t STEP_GROUPS_MAX_WALKERS = (\d+);", fh.read()).group(1))


@pytest.mark.gpu
def test_form_follows_the_previous_calls_walkers(world, monkeypatch, capfd):
    """A batch FULL of walkers is cheaper lane = read: the host picks the form from the plain walkers of the handle's
    previous call.  Few, many, many, few, few on one handle: groups, groups, lane = read, lane = read, groups -- and
    every call equal to the checker, whatever the hint said."""
    tree, cap = world["g"].tree, max_group_walkers()
    walkers = np.flatnonzero((world["events"] >= 1) & (world["events"] <= WALK_LIMIT))
    few, many = walkers[:500], np.resize(walkers, cap + 1000)
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    mat = w.Mat(tree)
    try:
        seen = []
        for idx in (few, many, many, few, few):
            res = mat.place_batch(rk.take(world["reads"], idx))
            seen.append(step_form(capfd))
            assert_checker(res, sub(world["want"], idx), f"call {len(seen)}")
        assert seen == [(8, 0), (8, few.size), (0, many.size), (0, many.size), (8, few.size)], seen
    finally:
        mat.close()


def turning_samples(tree, n, seed):
    """n reads of 8 entries at positions with 2 - 8 mutations, the first in front of position 1 024 and the last behind
    2 560, so that no genome window holds the read and it keeps most of its 16 - 64 events in a tree-wide stream."""
    counts, ref = position_table(tree)
    rng = np.random.default_rng(seed)
    hot = np.flatnonzero((counts >= 2) & (counts <= 8))
    lo, mid, hi = hot[hot < 1024], hot[(hot >= 1024) & (hot < 2560)], hot[hot >= 2560]
    out = []
    for _ in range(n):
        pos = np.sort(np.concatenate([rng.choice(lo, 1), rng.choice(mid, WALK8_K - 2, replace=False), rng.choice(hi, 1)]))
        out.append([entry(rng, p, ref) for p in pos])
    return out


WW_CALL_MAX_SMALL = 16384       # device_mat.hpp: reads with 17 .. 64 events in a call beyond which the next call goes by jobs


@pytest.mark.gpu
def test_groups_of_16_on_a_handle_that_turned_to_jobs(world, monkeypatch, capfd):
    """G = 16 as a handle reaches it by itself: a call full of reads with 7 - 64 events turns the handle to jobs
    (ww_by_jobs), the NEXT call lets up to 16 events walk plainly and places them by groups of 16 lanes, and the call
    after that is back at 6 events and groups of 8.  Every call against the checker."""
    tree, model, inc = world["g"].tree, world["model"], world["inc"]
    turn = turning_samples(tree, 22_000, SEED + 20)
    ev = np.array([model.events_of(S) for S in turn])
    assert ((ev > WALK_LIMIT) & (ev <= 64)).sum() > WW_CALL_MAX_SMALL + 500, np.bincount(np.minimum(ev, 70)).tolist()
    turn_reads = Reads.from_lists(turn)
    reads, events, ks = world["reads"], world["events"], world["ks"]
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    mat = w.Mat(tree)
    try:
        res = mat.place_batch(turn_reads)
        c1, step = debug_lines(capfd)
        assert step == (8, 0), step
        assert_checker(res, inc.place_batch(turn_reads, nthreads=NTHREADS), "the call that turns the handle")
        res = mat.place_batch(reads)
        c2, step = debug_lines(capfd)
        assert step == (16, c1["walk8"]), (step, c1)
        assert c2["walk8"] == int(((events >= 1) & (events <= WALK_LIMIT_WIDE) & (ks <= WALK8_K)).sum()), c2
        assert_checker(res, world["want"], "groups of 16 behind it")
        res = mat.place_batch(reads)
        c3, step = debug_lines(capfd)
        assert step == (8, c2["walk8"]), (step, c2)
        assert c3["walk8"] == int(((events >= 1) & (events <= WALK_LIMIT) & (ks <= WALK8_K)).sum()), c3
        assert_checker(res, world["want"], "groups of 8 again")
    finally:
        mat.close()
