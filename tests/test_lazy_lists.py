"""The grouped read list of a placement call (capi.cpp: k_scatter) is made only when a launch reads it: the routing
counters reach the host first, k_scatter runs BLIND behind their copy when the handle's previous call had consumers
(the hint expect_lists), LATE when the hint said no and the counters say yes, and not at all otherwise -- and then the
plan stream is not joined into the caller's stream either.  WEPP_DEBUG_PLANS=1 prints which it was ("[lists]").

The tree has 60 000 nodes; WEPP_SEED_MIN_NODES=0 lets whole-genome samples be seeded on it.  Two batches:
  A  reads that k_route, the plain walk and the wave role of k_step place: nothing reads the list;
  B  A's reads mixed with reads of every consumer: plain sweeps, sweeps of a window crown (k_sweep_arena), window
     tiles, seeded samples (near and far), and a chunked walk class that outgrows its blind tables, which the host
     then plans itself (more than 32 768 reads of it: a few hundred distinct reads, repeated).
Which read is of which class is taken from a probe handle's last_plans, never guessed, and asserted again on the call
under test.  The incremental checker is the reference, computed once for the distinct reads and shared."""
import os
import re

import numpy as np
import pytest

import read_kinds as rk
import wepp_amd as w
from wepp_amd import Reads

pytestmark = pytest.mark.gpu
NTHREADS = min(16, os.cpu_count() or 1)
FIELDS = ("best_bfs_j", "score", "num_best", "flags")
BLIND_CHUNKED_READS = 32768     # device_mat.hpp: reads of a chunked class k_route's blind tables hold
LISTS_LINE = re.compile(r"\[lists\] scatter=(none|blind|late) plan stream joined=([01])")
ROUTE_LINE = re.compile(r"\[route\] reads=(\d+) resolved=(\d+) walk=(\d+),(\d+) wave=(\d+),(\d+) .* job reads=(\d+),(\d+) jobs=(\d+),(\d+) left to the host=(\d+),(\d+)")
CONSUMERS = ("sweep", "arena", "window", "seed")


def new_mat(tree, **env):
    """A handle that prints its routing and seeds samples on a small tree, with the given environment besides (read
    once, when the handle is created)."""
    env = {"WEPP_DEBUG_PLANS": "1", "WEPP_SEED_MIN_NODES": "0", **env}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return w.Mat(tree)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def debug_lines(capfd):
    """([lists] lines as (mode, joined), [route] lines as dicts) printed since the last look"""
    err = capfd.readouterr().err
    lists = [(m, int(j)) for m, j in LISTS_LINE.findall(err)]
    routes = []
    for v in ROUTE_LINE.findall(err):
        v = [int(x) for x in v]
        routes.append(dict(reads=v[0], resolved=v[1], walk8=v[2], walk16=v[3], wave=v[4] + v[5], job_reads=v[6] + v[7], host=v[10] + v[11]))
    return lists, routes


def n_only_reads(rng, n, genome_len=rk.GENOME):
    """Samples of 20 - 30 N entries all over the genome: too many entries to walk, no window holds them, no entry that
    excludes a base for the seeds: plain sweeps of the tree-wide stream (PLAN_SWEEP)."""
    samples = []
    for _ in range(n):
        pos = np.sort(rng.choice(np.arange(1, genome_len + 1), size=int(rng.integers(20, 31)), replace=False))
        samples.append([(int(p), 1 << int(rng.integers(0, 4)), 15, 1) for p in pos])
    return Reads.from_lists(samples)


def want_of(want, idx):
    """the checker's records (a structured array) of the reads idx"""
    return want[np.asarray(idx, np.int64)]


def assert_checker(res, want, ctx):
    for name, got, exp in (("score", res.score, want["score"]), ("best_bfs_j", res.best_bfs_j, want["best_j"]),
                           ("num_best", res.num_best, want["num_best"]), ("has_unique", res.has_unique, want["has_unique"])):
        bad = np.flatnonzero(np.asarray(got) != np.asarray(exp))
        assert bad.size == 0, f"{ctx}: {name} differs at reads {bad[:10].tolist()}"


def assert_equal(got, want, ctx):
    for f in FIELDS:
        a, b = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{ctx}: {f} differs at {bad.size} reads, first {bad[:8].tolist()} (got {a[bad[:4]].tolist()}, want {b[bad[:4]].tolist()})"


def consumer_masks(cls, st):
    crown = st == w.WINDOW_CROWN_SLOT
    return {"sweep": (cls == w.PLAN_SWEEP) & ~crown, "arena": (cls == w.PLAN_SWEEP) & crown, "window": cls == w.PLAN_WIN,
            "seed": cls == w.PLAN_SEED}


@pytest.fixture(scope="module")
def world(oracle):
    """The tree, the distinct reads U with the checker's results, A and B as index lists into U, and both batches placed
    alone on a handle that always launches k_scatter blind (the form before the lists became lazy)."""
    g = w.generate_tree(33, 60_000)
    rng = np.random.default_rng(77)
    pool = rk.concat([
        g.reads(34, 8000, p_substitution=0.003, p_n=0.02, p_iupac=0.1),                  # plain walkers
        rk.hot_position_reads(g.tree, rng, 600, hot=400, k_lo=2, k_hi=6),                 # tens of events: the wave role
        g.reads(35, 1500, p_n=0.10), g.reads(36, 1000, p_substitution=0.01, p_n=0.20),    # 17 - 32 entries: sweeps of a crown
        n_only_reads(rng, 200),                                                           # plain sweeps
        rk.long_reads(g, 37, 400),                                                        # window tiles
        rk.genome_samples(g, 38, 60), rk.far_samples(rng, 40),                            # seeded
        rk.hot_position_reads(g.tree, rng, 400, hot=60, k_lo=12, k_hi=16),                # ~1000 events: jobs
    ])
    probe = new_mat(g.tree)
    probe.set_pipeline(1)
    probe.place_batch(pool)
    cls, st = probe.last_plans(pool.n_reads)
    probe.close()
    k = np.diff(pool.read_off.astype(np.int64))
    print("pool classes", np.bincount(cls, minlength=7).tolist(), {n: int(m.sum()) for n, m in consumer_masks(cls, st).items()})
    first_hot = 8000
    plain = np.flatnonzero((cls == w.PLAN_WALK8) & (np.arange(pool.n_reads) < first_hot))[:3000]
    empty = np.flatnonzero((k == 0) & (np.arange(pool.n_reads) < first_hot))[:50]
    # (at most 256 events in the tree-wide stream, so in any stream: the wave role takes them, never the job tables)
    mut_pos = np.asarray(g.tree.mut_pos)
    per_pos = np.bincount(mut_pos[mut_pos >= 0], minlength=rk.GENOME + 2)
    events = np.array([int(per_pos[pool.entries(r)[0]].sum()) for r in range(first_hot, first_hot + 600)])
    waves = first_hot + np.flatnonzero((cls[first_hot:first_hot + 600] == w.PLAN_WALKC8) & (events <= 256))[:300]
    assert plain.size == 3000 and waves.size >= 50, (plain.size, waves.size)
    a_pool = np.unique(np.concatenate([plain, empty, waves]))
    picks = {}
    for name, m in consumer_masks(cls, st).items():
        picks[name] = np.flatnonzero(m)[:300]
        assert picks[name].size > 0, f"no {name} read in the pool: {np.bincount(cls, minlength=7).tolist()}"
    jobs = np.flatnonzero(((cls == w.PLAN_WALKC8) | (cls == w.PLAN_WALKC16)) & (np.arange(pool.n_reads) >= pool.n_reads - 400))
    assert jobs.size >= 100, jobs.size
    # U = the distinct reads, A first; the checker places each once
    u_idx = np.concatenate([a_pool] + [picks[n] for n in CONSUMERS] + [jobs])
    U = rk.take(pool, u_idx)
    nA = a_pool.size
    inc = oracle.OracleTree(g.tree).incremental()
    want_u = inc.place_batch(U, nthreads=NTHREADS)
    a_idx = np.random.default_rng(5).permutation(nA)
    lo = nA + sum(picks[n].size for n in CONSUMERS)
    b_idx = np.concatenate([np.arange(lo), np.resize(np.arange(lo, U.n_reads), BLIND_CHUNKED_READS + 700)])
    b_idx = np.random.default_rng(6).permutation(b_idx)
    A, B = rk.take(U, a_idx), rk.take(U, b_idx)
    assert B.n_reads < 65_536        # (one device call per place_batch)
    one = {n: rk.take(U, [nA + sum(picks[m].size for m in CONSUMERS[:i])]) for i, n in enumerate(CONSUMERS)}
    blind = new_mat(g.tree, WEPP_SCATTER_BLIND="1")
    blind.set_pipeline(1)
    alone = {"A": blind.place_batch(A), "B": blind.place_batch(B)}
    blind.close()
    yield dict(g=g, inc=inc, A=A, B=B, want={"A": want_of(want_u, a_idx), "B": want_of(want_u, b_idx)}, alone=alone, one=one)
    g.close()


def assert_b_is_populated(mat, B, route):
    """every consumer class holds reads in the call just made, and a chunked class was left to the host's plans"""
    cls, st = mat.last_plans(B.n_reads)
    for name, m in consumer_masks(cls, st).items():
        assert m.sum() > 0, (name, np.bincount(cls, minlength=7).tolist())
    assert route["host"] > 0 and route["job_reads"] > BLIND_CHUNKED_READS, route


def test_hint_sequence_on_one_handle(world, capfd):
    """A, A, B, B, A, B, A on one handle: no k_scatter, none, late, blind, blind (the hint of B, for nothing), late, none
    (a blind launch for nothing keeps the next B from setting the hint: batches of both kinds in turn do not pay an idle
    kernel in front of every A) -- the plan stream joined exactly when the kernel ran --, every call equal to the checker and to the same call on a
    handle with WEPP_SCATTER_BLIND=1 and on one with WEPP_STEP_UNFUSED=1."""
    g, order = world["g"], "AABBABA"
    debug_lines(capfd)
    mat = new_mat(g.tree)
    mat.set_pipeline(1)
    try:
        got, lists, routes = [], [], []
        for x in order:
            got.append(mat.place_batch(world[x]))
            ls, rs = debug_lines(capfd)
            assert len(ls) == 1 and len(rs) == 1, (ls, rs)
            lists.append(ls[0])
            routes.append(rs[0])
            if x == "B":
                assert_b_is_populated(mat, world["B"], rs[0])
            else:
                cls, _ = mat.last_plans(world["A"].n_reads)
                assert set(np.unique(cls).tolist()) == {w.PLAN_WALK8, w.PLAN_WALKC8}, np.bincount(cls).tolist()
                assert rs[0]["walk8"] > 0 and rs[0]["host"] == 0, rs[0]
        print(lists, routes)
        assert routes[0]["wave"] > 0 and routes[0]["job_reads"] == 0, routes[0]     # (A's many-event reads went to the wave role)
        assert [m for m, _ in lists] == ["none", "none", "late", "blind", "blind", "late", "none"], lists
        assert [j for _, j in lists] == [0, 0, 1, 1, 1, 1, 0], lists
        for mode in ("late", "blind"):          # (... and two B in a row set the hint again)
            assert_equal(mat.place_batch(world["B"]), world["alone"]["B"], f"B again ({mode})")
            assert debug_lines(capfd)[0] == [(mode, 1)]
        for i, x in enumerate(order):
            assert_checker(got[i], world["want"][x], f"call {i} ({x})")
            assert_equal(got[i], world["alone"][x], f"call {i} ({x}) vs WEPP_SCATTER_BLIND=1")
    finally:
        mat.close()
    for env in ({"WEPP_SCATTER_BLIND": "1"}, {"WEPP_STEP_UNFUSED": "1"}):
        m2 = new_mat(g.tree, **env)
        m2.set_pipeline(1)
        try:
            debug_lines(capfd)
            for i, x in enumerate(order):
                assert_equal(m2.place_batch(world[x]), got[i], f"call {i} ({x}) with {env}")
            ls, _ = debug_lines(capfd)
            assert ls == [("blind", 1)] * len(order), (env, ls)
        finally:
            m2.close()


def test_back_to_back_without_host_synchronisation(world, capfd):
    """Six device-pointer calls alternating A and B on one stream, each into result tensors of its own, one
    synchronisation at the end: every call's four arrays are those of the batch placed alone.  (A late consumer of call
    N that was not joined would read routing buffers call N + 1 rewrote; the counter sets alternate.)"""
    import torch
    g = world["g"]
    dev = torch.device("cuda", 0)
    mat = new_mat(g.tree)
    try:
        d_in = {}
        for x in "AB":
            r = world[x]
            d_in[x] = (torch.from_numpy(r.read_off.astype(np.int32)).to(dev), torch.from_numpy(r.read_word.astype(np.int32)).to(dev))
        order = "ABABAB"
        outs = [[torch.full((world[x].n_reads,), -1, dtype=torch.int32, device=dev) for _ in range(4)] for x in order]
        # (a warm-up call of B first: the workspace has its final size, so no call below synchronises to regrow it)
        warm = [torch.zeros(world["B"].n_reads, dtype=torch.int32, device=dev) for _ in range(4)]
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            mat.place_batch_device(d_in["B"][0].data_ptr(), d_in["B"][1].data_ptr(), world["B"].n_reads, int(world["B"].read_off[-1]),
                                   *[o.data_ptr() for o in warm], stream.cuda_stream)
        stream.synchronize()
        mat.place_batch(rk.empty_reads(8))      # (... and no consumers expected, after a blind k_scatter for nothing)
        debug_lines(capfd)
        with torch.cuda.stream(stream):
            for x, o in zip(order, outs):
                r = world[x]
                mat.place_batch_device(d_in[x][0].data_ptr(), d_in[x][1].data_ptr(), r.n_reads, int(r.read_off[-1]),
                                       *[t.data_ptr() for t in o], stream.cuda_stream)
        stream.synchronize()
        ls, _ = debug_lines(capfd)
        # (the warm-up left the hint "the last blind launch found nothing": the first B does not set it, the second does)
        assert [m for m, _ in ls] == ["none", "late", "none", "late", "blind", "late"], ls
        for i, (x, o) in enumerate(zip(order, outs)):
            alone = world["alone"][x]
            for f, t in zip(FIELDS, o):
                a, b = t.cpu().numpy().view(np.uint32), np.asarray(getattr(alone, f)).view(np.uint32)
                bad = np.flatnonzero(a != b)
                assert bad.size == 0, f"call {i} ({x}): {f} differs at {bad.size} reads, first {bad[:8].tolist()}"
    finally:
        mat.close()


def test_two_lanes(world):
    """concat([A, B, A, B]) in two sub-batches, one per lane (each with its own counters, event and plan stream; the
    hint is the handle's), against the unsplit call and the checker."""
    g = world["g"]
    both = rk.concat([world[x] for x in "ABAB"])
    assert both.n_reads >= 65_536          # (a pipelined call)
    mat = new_mat(g.tree)
    try:
        mat.set_pipeline(1)
        whole = mat.place_batch(both)
        mat.set_pipeline(2)
        split = mat.place_batch(both)
        assert_equal(split, whole, "two sub-batches")
        lo = 0
        for i, x in enumerate("ABAB"):
            n = world[x].n_reads
            sub = w.PlacementResult(*(np.asarray(getattr(split, f))[lo:lo + n] for f in FIELDS))
            assert_checker(sub, world["want"][x], f"two sub-batches, part {i} ({x})")
            lo += n
    finally:
        mat.close()


def test_edges(world, capfd):
    """A batch of empty reads (all resolved by k_route: no k_scatter, no join); A with the walks off (everything is
    listed and the plan stream is the caller's stream: blind, nothing to join); one read of each consumer class alone
    on a fresh handle (late, a list of one read)."""
    g, inc = world["g"], world["inc"]
    debug_lines(capfd)
    mat = new_mat(g.tree)
    try:
        empty = rk.empty_reads(500)
        res = mat.place_batch(empty)
        ls, rs = debug_lines(capfd)
        assert ls == [("none", 0)] and rs[0]["resolved"] == 500, (ls, rs)
        assert_checker(res, inc.place_batch(empty, nthreads=NTHREADS), "empty reads")
        mat.set_use_walk(False)
        res = mat.place_batch(world["A"])
        ls, _ = debug_lines(capfd)
        assert ls == [("blind", 0)], ls
        assert_checker(res, world["want"]["A"], "A, walks off")
    finally:
        mat.close()
    for name, read in world["one"].items():
        want = inc.place_batch(read, nthreads=1)
        m1 = new_mat(g.tree)
        try:
            debug_lines(capfd)
            res = m1.place_batch(read)
            ls, _ = debug_lines(capfd)
            cls, st = m1.last_plans(1)
            assert consumer_masks(cls, st)[name].all(), (name, cls, st)
            assert ls == [("late", 1)], (name, ls)
            assert_checker(res, want, f"one {name} read")
        finally:
            m1.close()
