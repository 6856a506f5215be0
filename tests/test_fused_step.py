"""k_step: the plain walkers and the reads with many events of a placement call in one launch behind k_route
(walk_kernels.hip), the pair pass of a large read cut into slices over the waves of a workgroup (place_dev.hpp:
wave_read), and the 8-entry job class launched from a hint (capi.cpp: expect_jobs8).

The tree is the one of test_reads_with_many_events_vs_oracle: 60 000 nodes over 1 500 positions, ~40 mutations per
position at the median.  Its least mutated position carries 7 mutations, so a read's summed per-position mutation count
-- its events in the tree-wide stream -- starts at 7: the ladder below holds every total from 7 to 300, three reads
each (totals of 1 - 6 do not exist on this tree; reads routed to a crown have fewer events in THEIR stream than the
total, which is how the batch crosses 6 / 7 as well: both walk8 and walkc8 must be populated).  The incremental
checker is the reference; its results are computed once per module."""
import os
import re

import numpy as np
import pytest

import read_kinds as rk
import sweep_model as sm
import walk_model as wm
import wepp_amd as w
from wepp_amd import Reads

NTHREADS = min(16, os.cpu_count() or 1)
FIELDS = ("best_bfs_j", "score", "num_best", "flags")
LADDER_MAX = 300
PER_TOTAL = 3
# every size at which the placement takes another path: walk -> wave pass (6 / 7, in the read's own stream), one wave ->
# the waves of a workgroup (64 / 65), the slices of the pair pass (128 / 129: two rows -> three rows in two slices,
# 192 / 193: -> four rows), wave pass -> jobs (256 / 257)
BOUNDARIES = (7, 8, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 194, 255, 256, 257, 258)


def wave_role_workgroups():
    """STEP_WAVE_WGS of device_mat.hpp: the most workgroups of k_step that take the wave role."""
    path = os.path.join(os.path.dirname(os.path.abspath(w.__file__)), "csrc", "device_mat.hpp")
    with open(path) as fh:
        return int(re.search(r"constexpr uint32_t STEP_WAVE_WGS = (\d+);", fh.read()).group(1))


def make_tree():
    return w.generate_tree(61, 60_000, genome_len=1500, p_ambiguous=0.02, p_masked_node=0.003, root_mutations=1)


def position_table(tree):
    """(mutations per position, reference allele per position) of the tree."""
    pos = np.asarray(tree.mut_pos)
    keep = pos >= 0
    counts = np.bincount(pos[keep])
    ref = np.zeros(counts.size, np.int64)
    ref[pos[keep]] = np.asarray(tree.mut_ref)[keep]
    return counts, ref


def entry(rng, p, ref):
    """half concrete alleles, a fifth ambiguity codes, the rest N"""
    u = rng.random()
    if u < 0.5:
        return (int(p), int(ref[p]), 1 << int(rng.integers(0, 4)), 0)
    if u < 0.7:
        return (int(p), int(ref[p]), int(rng.integers(1, 15)), 0)
    return (int(p), int(ref[p]), 15, 1)


def read_with_total(rng, counts, ref, by_count, total):
    """A read of 1 - 8 entries at distinct positions whose mutation counts sum to `total`."""
    mutated = np.flatnonzero(counts > 0)
    for _ in range(10_000):
        k = int(rng.integers(1, 9))
        first = rng.choice(mutated, size=k - 1, replace=False) if k > 1 else np.zeros(0, np.int64)
        rest = total - int(counts[first].sum())
        last = [p for p in by_count.get(rest, ()) if p not in first]
        if rest > 0 and last:
            pos = np.sort(np.append(first, last[int(rng.integers(0, len(last)))]))
            assert int(counts[pos].sum()) == total and len(set(pos.tolist())) == len(pos)
            return [entry(rng, p, ref) for p in pos]
    raise AssertionError(f"no read with {total} events found")


def ladder_reads(tree, totals, per_total=PER_TOTAL, seed=5):
    counts, ref = position_table(tree)
    by_count = {}
    for p in np.flatnonzero(counts > 0):
        by_count.setdefault(int(counts[p]), []).append(int(p))
    rng = np.random.default_rng(seed)
    samples, total_of = [], []
    for t in totals:
        for _ in range(per_total):
            samples.append(read_with_total(rng, counts, ref, by_count, t))
            total_of.append(t)
    return samples, np.array(total_of)


def reads_in_range(tree, n, lo, hi, seed):
    """n reads whose totals are spread over lo .. hi"""
    totals = np.resize(np.arange(lo, hi + 1), n) if n >= hi + 1 - lo else np.linspace(lo, hi, n).astype(np.int64)
    samples, _ = ladder_reads(tree, totals, per_total=1, seed=seed)
    return samples


def assert_checker(res, want, ctx):
    for name, got, exp in (("score", res.score, want["score"]), ("best_bfs_j", res.best_bfs_j, want["best_j"]),
                           ("num_best", res.num_best, want["num_best"]), ("has_unique", res.has_unique, want["has_unique"])):
        bad = np.flatnonzero(np.asarray(got) != np.asarray(exp))
        assert bad.size == 0, f"{ctx}: {name} differs at reads {bad[:10].tolist()} (gpu {np.asarray(got)[bad[:5]]}, checker {np.asarray(exp)[bad[:5]]})"


def assert_equal(got, want, ctx):
    for f in FIELDS:
        a, b = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{ctx}: {f} differs at {bad.size} reads, first {bad[:8].tolist()} (got {a[bad[:4]].tolist()}, want {b[bad[:4]].tolist()})"


def test_ladder_covers_every_total_and_model_equals_checker(oracle):
    """On the CPU: the ladder holds every total the tree allows, three reads each, and at every boundary total the
    all-pairs model of the wave pass (tests/walk_model.py: place_all_pairs, on the tree-wide stream, where a read's
    events ARE its total, and on the stream the read is routed to) places the reads as the incremental checker does."""
    g = make_tree()
    counts, _ = position_table(g.tree)
    low = int(counts[counts > 0].min())
    assert low == 7, low                       # (totals below do not exist on this tree: see the module's docstring)
    samples, total_of = ladder_reads(g.tree, range(low, LADDER_MAX + 1))
    assert np.bincount(total_of, minlength=LADDER_MAX + 1)[low:].min() >= PER_TOTAL
    ks = {len(s) for s in samples}
    assert ks == set(range(1, 9)), ks
    assert {e[3] for s in samples for e in s} == {0, 1} and any(e[2] not in (1, 2, 4, 8, 15) for s in samples for e in s)
    fv = w.FlatView(g.tree)
    inc = oracle.OracleTree(g.tree).incremental()
    tiers = sm.TieredModel(fv)
    models = {}
    n = 0
    for i in np.flatnonzero(np.isin(total_of, [t for t in BOUNDARIES if t <= 256])):
        S = samples[i]
        o = inc.place_sample(*(list(c) for c in zip(*S)))
        rs = sm.theta(fv, S) - len(S)
        for stream in {fv.n_streams - 1, tiers.route(S)}:
            m = models.get(stream) or models.setdefault(stream, wm.WalkModel(fv, stream))
            if stream == fv.n_streams - 1:
                assert m.events_of(S) == total_of[i], (S, m.events_of(S), total_of[i])
            bs, br, cnt, hu = m.place_all_pairs(S, rs)
            assert (bs, int(m.rank2bfs[br]), cnt, hu) == (o["score"], o["best_j"], o["num_best"], o["has_unique"]), (S, stream)
        n += 1
    assert n >= PER_TOTAL * 16


@pytest.fixture(scope="module")
def world(oracle):
    """The tree, its checker, and the ladder batch with the checker's results."""
    g = make_tree()
    inc = oracle.OracleTree(g.tree).incremental()
    counts, _ = position_table(g.tree)
    samples, total_of = ladder_reads(g.tree, range(int(counts[counts > 0].min()), LADDER_MAX + 1))
    reads = Reads.from_lists(samples)
    want = inc.place_batch(reads, nthreads=NTHREADS)
    yield dict(g=g, inc=inc, reads=reads, want=want, total_of=total_of)
    g.close()


@pytest.mark.gpu
def test_event_count_ladder(world, monkeypatch):
    """Every total from the tree's minimum to 300: against the checker, and the same four arrays from the three
    launches k_step replaced, from a handle that cuts every such read into jobs, and with the walks off."""
    g, reads = world["g"], world["reads"]
    mat = w.Mat(g.tree)
    res = mat.place_batch(reads)
    cls, _ = mat.last_plans(reads.n_reads)
    assert (cls == w.PLAN_WALK8).sum() > 0 and (cls == w.PLAN_WALKC8).sum() > 0, np.bincount(cls).tolist()
    assert_checker(res, world["want"], "ladder")
    mat.set_use_walk(False)
    try:
        assert_equal(mat.place_batch(reads), res, "ladder: walks off")
    finally:
        mat.set_use_walk(True)
    mat.close()
    for env, ctx in (({"WEPP_STEP_UNFUSED": "1"}, "three launches"),
                     ({"WEPP_WW_BLOCK_MAX_SMALL": "0", "WEPP_WW_BLOCK_MAX_BIG": "0"}, "all by jobs")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m2 = w.Mat(g.tree)           # (the switches are read when the handle is created)
        try:
            assert_equal(m2.place_batch(reads), res, f"ladder: {ctx}")
        finally:
            m2.close()


ROUTE_LINE = re.compile(r"\[route\] reads=(\d+) resolved=(\d+) walk=(\d+),(\d+) wave=(\d+),(\d+) \(of them walkers of 9 - 16 entries: (\d+)\) "
                        r"job reads=(\d+),(\d+)")


def route_counts(capfd):
    """k_route's counters of the last call of a handle created with WEPP_DEBUG_PLANS=1 (capi.cpp prints them): reads,
    placed by k_route itself, plain walkers of 1 - 8 / 9 - 16 entries, wave-pass reads of <= 64 / more events, ..."""
    lines = ROUTE_LINE.findall(capfd.readouterr().err)
    assert lines, "no [route] line"
    v = [int(x) for x in lines[-1]]
    return dict(reads=v[0], resolved=v[1], walk8=v[2], walk16=v[3], wave_small=v[4], wave_big=v[5], jobs8=v[7], jobs16=v[8])


@pytest.mark.gpu
def test_role_edges_of_the_fused_launch(world, monkeypatch, capfd):
    """Batches that leave one role of k_step without work, or give it more than its workgroups: each on a fresh handle
    (no hint from a call before), each against the checker.  What k_route made of a batch -- how many plain walkers, how
    many reads for the wave role and of which size -- is read from the counters it leaves (WEPP_DEBUG_PLANS prints
    them), not guessed from the reads: a read routed to a crown has fewer events in its stream than in the tree."""
    g, inc = world["g"], world["inc"]
    wave_wgs = wave_role_workgroups()
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    probe = w.Mat(g.tree)

    def counts_of(reads):
        probe.place_batch(reads)
        return route_counts(capfd)

    # plain walkers: on this tree every listed position is mutated at least 7 times, so a read walks plainly only in a
    # crown that holds few of those mutations: the reads of the first plain class among 6 000 drawn from the leaves
    pool = g.reads(18, 6000, read_len=150, amplicon_len=400, amplicon_step=300, p_substitution=0.002, p_n=0.0)
    probe.place_batch(pool)
    pool_cls, _ = probe.last_plans(pool.n_reads)
    plain = rk.take(pool, np.flatnonzero((pool_cls == w.PLAN_WALK8) & (np.diff(pool.read_off.astype(np.int64)) > 0))[:2000])
    assert plain.n_reads == 2000
    # reads of the wave role: of 1 500 with 100 - 256 events in the tree those of a chunked class
    cand = Reads.from_lists(reads_in_range(g.tree, 1500, 100, 256, seed=19))
    probe.place_batch(cand)
    cand_cls, _ = probe.last_plans(cand.n_reads)
    many = rk.take(cand, np.flatnonzero(cand_cls == w.PLAN_WALKC8))
    # one read the wave role gives a whole workgroup: placed alone, k_route counts it among those with more than 64 events
    one_big = next((r for r in (rk.take(many, [i]) for i in range(many.n_reads - 1, many.n_reads - 60, -1)) if counts_of(r)["wave_big"] == 1), None)
    assert one_big is not None
    probe.close()
    # (1 500 distinct reads with 200 - 256 events in the tree, repeated: about two in five keep more than 64 in their stream)
    wrap = Reads.from_lists(reads_in_range(g.tree, 1500, 200, 256, seed=21))
    wrap = rk.take(wrap, np.resize(np.arange(wrap.n_reads), 3 * wave_wgs))
    batches = {
        "no events": rk.empty_reads(500),
        "plain walkers": plain,
        "many-event reads": many,
        "one large read among plain walkers": rk.concat([rk.take(plain, np.arange(1000)), one_big, rk.take(plain, np.arange(1000, 2000))]),
        "more large reads than wave-role workgroups": wrap,
    }
    for name, reads in batches.items():
        want = inc.place_batch(reads, nthreads=NTHREADS)
        mat = w.Mat(g.tree)
        try:
            res = mat.place_batch(reads)
            c = route_counts(capfd)
            print(name, c)
            assert_checker(res, want, name)
            assert c["reads"] == reads.n_reads
            if name == "no events":
                assert c["resolved"] == reads.n_reads, c
            elif name == "plain walkers":
                assert c["walk8"] > 0 and c["walk8"] + c["resolved"] == reads.n_reads and c["wave_small"] + c["wave_big"] == 0, c
            elif name == "many-event reads":
                assert c["walk8"] == 0 and c["resolved"] == 0 and c["wave_small"] > 0 and c["wave_big"] > 0, c
            elif name == "one large read among plain walkers":
                assert (c["wave_small"], c["wave_big"]) == (0, 1) and c["walk8"] > 0 and c["jobs8"] == 0, c
            else:
                assert c["wave_big"] > wave_wgs, (c, wave_wgs)
        finally:
            mat.close()


@pytest.mark.gpu
def test_hint_sequence_on_one_handle(world, monkeypatch, capfd):
    """A (plain walkers and a few reads with many events) and B (full of such reads: it turns the handle to jobs and
    makes it expect the job class) in turn on one handle: A, B, A, B.  Both placements of each are identical and equal
    to the checker's, and k_route's counters show that A went by waves first and by jobs after B; then a batch large
    enough to be split, such reads in both halves, in two sub-batches against the unsplit call."""
    g, inc = world["g"], world["inc"]
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    pool = g.reads(31, 64_000, read_len=150, amplicon_len=400, amplicon_step=300, p_substitution=0.002, p_n=0.01)
    mat = w.Mat(g.tree)
    try:
        mat.place_batch(pool)
        pool_cls, _ = mat.last_plans(pool.n_reads)
        plain = rk.take(pool, np.flatnonzero(pool_cls == w.PLAN_WALK8)[:24_000])
        assert plain.n_reads == 24_000
        few = Reads.from_lists(reads_in_range(g.tree, 40, 7, 300, seed=32) + reads_in_range(g.tree, 20, 400, 900, seed=34))
        a = rk.concat([rk.take(plain, np.arange(12_000)), few, rk.take(plain, np.arange(12_000, 24_000))])
        b = rk.concat([rk.take(pool, np.flatnonzero(pool_cls == w.PLAN_WALKC8)), Reads.from_lists(reads_in_range(g.tree, 3000, 100, 300, seed=33))])
        want_a, want_b = inc.place_batch(a, nthreads=NTHREADS), inc.place_batch(b, nthreads=NTHREADS)
        mat.place_batch(rk.empty_reads(8))          # (the hints of a fresh handle again: no such reads in the call before)
        got, counts = [], []
        for x in (a, b, a, b):
            got.append(mat.place_batch(x))
            counts.append(route_counts(capfd))
        print(counts)
        assert_checker(got[0], want_a, "A, first")
        assert_checker(got[1], want_b, "B, first")
        assert_equal(got[2], got[0], "A after B")
        assert_equal(got[3], got[1], "B after A")
        # A holds reads for both the wave role and the job class; after B its wave lists are empty and its jobs more
        assert counts[0]["wave_small"] + counts[0]["wave_big"] > 0 and counts[0]["jobs8"] > 0, counts[0]
        assert counts[2]["wave_small"] + counts[2]["wave_big"] == 0 and counts[2]["jobs8"] > counts[0]["jobs8"], counts[2]
        assert counts[1] == counts[3] and counts[1]["wave_small"] + counts[1]["wave_big"] > 2048 and counts[1]["jobs8"] > 0, counts[1]
        both = rk.concat([a, b, a, b])
        whole = mat.place_batch(both)
        mat.set_pipeline(2)
        try:
            split = mat.place_batch(both)
        finally:
            mat.set_pipeline(0)
        assert_equal(split, whole, "two sub-batches")
        lo = 0
        for i, (x, wn) in enumerate(((a, want_a), (b, want_b), (a, want_a), (b, want_b))):
            sub = w.PlacementResult(*(np.asarray(getattr(whole, f))[lo:lo + x.n_reads] for f in FIELDS))
            assert_checker(sub, wn, f"unsplit call, part {i}")
            lo += x.n_reads
    finally:
        mat.close()
