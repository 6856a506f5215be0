"""Trees of other shapes than the generator's default (wepp_gen_tree_params: depth_choices, p_hub / n_hubs): root paths
of 60 - 100 mutations and polytomies of thousands of children, as real SARS-CoV-2 trees have.  They drive what the
default tree hardly touches: the chunked walks by jobs (ww_by_jobs), window crowns larger than the tree, and ties among
thousands of siblings (the (score, rank) tie-break, num_best, best_j_vec).

The incremental checker is the reference of the GPU tests; the CPU test below holds it to the faithful oracle on the
same shapes, which its fuzz equality (test_incremental.py) never had: uniform random trees have no large polytomies."""
import os
import time

import numpy as np
import pytest

import read_kinds as rk
import wepp_amd as w

NTHREADS = min(16, os.cpu_count() or 1)
FIELDS = ("best_bfs_j", "score", "num_best", "flags")
SHAPES = {
    "default": {},
    "deep3": {"depth_choices": 3},
    "star": {"p_hub": 0.5, "n_hubs": 16},
    "deep_bushy": {"depth_choices": 3, "p_hub": 0.3, "n_hubs": 16},
}
WALKC = (w.PLAN_WALKC8, w.PLAN_WALKC16)


def shape_tree(name, n_nodes):
    return w.generate_tree(71, n_nodes, p_ambiguous=0.01, p_masked_node=0.002, root_mutations=1, **SHAPES[name])


def check_shape(name, sh):
    """what makes each shape what it is (GenTree.shape() of the 300 000-node trees; the generator is deterministic)"""
    if name == "deep3":
        assert sh["path_mutations_median"] >= 60, sh
    elif name == "star":
        assert sh["max_children"] >= 9000, sh
    elif name == "deep_bushy":
        assert sh["max_children"] >= 5000 and sh["path_mutations_p95"] >= 40, sh


def mixed_reads(g, n_short, n_long, n_genome):
    return rk.concat([g.reads(72, n_short, p_substitution=0.004, p_n=0.02, p_iupac=0.1), rk.long_reads(g, 73, n_long),
                      rk.genome_samples(g, 74, n_genome)])


def assert_equal(got, want, ctx, idx=None):
    for f in FIELDS:
        a, b = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        if idx is not None:
            b = b[idx]
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{ctx}: {f} differs at {bad.size} reads, first {bad[:8].tolist()} (got {a[bad[:4]].tolist()}, want {b[bad[:4]].tolist()})"


def assert_checker(res, want, ctx):
    for name, got, exp in (("score", res.score, want["score"]), ("best_bfs_j", res.best_bfs_j, want["best_j"]),
                           ("num_best", res.num_best, want["num_best"]), ("has_unique", res.has_unique, want["has_unique"])):
        bad = np.flatnonzero(np.asarray(got) != np.asarray(exp))
        assert bad.size == 0, f"{ctx}: {name} differs at reads {bad[:10].tolist()} (gpu {np.asarray(got)[bad[:5]]}, checker {np.asarray(exp)[bad[:5]]})"


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_preconditions(name):
    check_shape(name, shape_tree(name, 300_000).shape())


@pytest.mark.parametrize("name", list(SHAPES))
def test_checker_equals_faithful_oracle_on_shapes(oracle, name):
    """30 000-node trees of every shape: the incremental checker against the faithful oracle on 20 short, 10 long and
    10 whole-genome reads, every field and the list of optimal nodes."""
    g = shape_tree(name, 30_000)
    reads = mixed_reads(g, 20, 10, 10)
    ot = oracle.OracleTree(g.tree)
    inc = ot.incremental()
    want = ot.place_batch(reads, 4)
    got = inc.place_batch(reads, nthreads=4)
    for f in want.dtype.names:
        assert (got[f] == want[f]).all(), (name, f, np.flatnonzero(got[f] != want[f])[:10].tolist())
    for q in range(reads.n_reads):
        a = inc.place_sample(*reads.entries(q), want_best_vec=True)["best_j_vec"]
        b = ot.place_sample(*reads.entries(q), want_best_vec=True)["best_j_vec"]
        assert a.tolist() == b.tolist(), (name, q)
    assert got["num_best"].max() > 1


@pytest.fixture(scope="module", params=list(SHAPES))
def shaped(request, oracle):
    """A 300 000-node tree of the shape, 20 000 short reads, 2 000 of 1.2 kb and 300 whole-genome samples, a fresh
    handle's results and plans, and the incremental checker's results."""
    name = request.param
    g = shape_tree(name, 300_000)
    check_shape(name, g.shape())
    reads = mixed_reads(g, 20_000, 2_000, 300)
    ot = oracle.OracleTree(g.tree)
    inc = ot.incremental()
    t0 = time.perf_counter()
    want = inc.place_batch(reads, nthreads=NTHREADS)
    print(f"{name}: checker, {reads.n_reads} reads in {time.perf_counter() - t0:.2f} s")
    mat = w.Mat(g.tree)
    res = mat.place_batch(reads)
    cls, _ = mat.last_plans(reads.n_reads)
    yield dict(name=name, g=g, reads=reads, ot=ot, inc=inc, want=want, mat=mat, res=res, cls=cls)
    mat.close()
    g.close()


@pytest.mark.gpu
def test_shape_vs_checker_and_oracle(shaped):
    """Every read against the incremental checker; eight (short, long and genome) against the faithful oracle."""
    s = shaped
    reads, res = s["reads"], s["res"]
    assert_checker(res, s["want"], f"{s['name']}: vs the incremental checker")
    assert (s["cls"][-300:] == w.PLAN_SEED).mean() > 0.9 and (s["cls"][20_000:22_000] == w.PLAN_WIN).mean() > 0.9
    short = np.arange(20_000)
    eight = np.concatenate([[int(short[np.argmax(res.num_best[:20_000])])], [0, 1, 2], [20_000, 21_999], [22_000, 22_299]])
    few = rk.take(reads, eight)
    sub = w.PlacementResult(*(np.asarray(getattr(res, f))[eight] for f in FIELDS))
    assert_checker(sub, s["ot"].place_batch(few, NTHREADS), f"{s['name']}: vs the faithful oracle")


@pytest.mark.gpu
def test_shape_switches_give_the_same_arrays(shaped):
    """Walks off, work skipping (crowns) off, seeds off: the same four arrays."""
    s = shaped
    mat, reads, res = s["mat"], s["reads"], s["res"]
    for what, on, off in (("walks", lambda: mat.set_use_walk(True), lambda: mat.set_use_walk(False)),
                          ("crowns", lambda: mat.set_use_crowns(True), lambda: mat.set_use_crowns(False)),
                          ("seeds", lambda: mat.set_use_seeds(True), lambda: mat.set_use_seeds(False))):
        off()
        try:
            got = mat.place_batch(reads)
        finally:
            on()
        assert_equal(got, res, f"{s['name']}: {what} off")


# Shapes on which last_plans shows no switch: no read of the batch has 7 - 16 events in its stream, so none changes its
# class when the handle goes by jobs.  Measured on the MI355X (chunked-class reads by waves -> after the switch):
# default 50 -> 50, deep3 0 -> 0 (no read of the batch is in a chunked class at all);
# star 9 600 -> 5 156 and deep_bushy 4 076 -> 983 do switch.
NO_SWITCH = {"default", "deep3"}


@pytest.mark.gpu
def test_shape_waves_vs_jobs(shaped, monkeypatch):
    """The reads with many events by waves (a fresh handle's first call) and by jobs: a handle forced into jobs, and
    the handle's own switch -- a different batch of the same size full of such reads first, then this one."""
    s = shaped
    g, reads, res, cls = s["g"], s["reads"], s["res"], s["cls"]
    with monkeypatch.context() as mp:
        mp.setenv("WEPP_WW_BLOCK_MAX_SMALL", "0")
        mp.setenv("WEPP_WW_BLOCK_MAX_BIG", "0")
        mj = w.Mat(g.tree)
    assert_equal(mj.place_batch(reads), res, f"{s['name']}: forced into jobs")
    mj.close()
    other = rk.hot_position_reads(g.tree, np.random.default_rng(75), reads.n_reads, hot=4000, k_lo=2, k_hi=4)
    ms = w.Mat(g.tree)
    ms.place_batch(other)
    got = ms.place_batch(reads)
    cls2, _ = ms.last_plans(reads.n_reads)
    ms.close()
    assert_equal(got, res, f"{s['name']}: after the handle's own switch")
    # by jobs, reads of 7 - 16 events walk plainly (capi.cpp: walk_limit): fewer chunked reads is the switch
    n1, n2 = int(np.isin(cls, WALKC).sum()), int(np.isin(cls2, WALKC).sum())
    print(f"{s['name']}: chunked-class reads {n1} by waves, {n2} after the switch")
    if s["name"] in NO_SWITCH:
        assert n2 == n1, (n1, n2)
    else:
        assert n2 < n1, (n1, n2)


@pytest.mark.gpu
def test_shape_best_nodes_of_the_largest_ties(shaped):
    """best_nodes of the 50 reads with the most optimal nodes against the checker's best_j_vec."""
    s = shaped
    mat, reads, res, inc = s["mat"], s["reads"], s["res"], s["inc"]
    top = np.argsort(-res.num_best.astype(np.int64), kind="stable")[:50]
    sub = rk.take(reads, top)
    got = mat.best_nodes(sub, w.PlacementResult(*(np.asarray(getattr(res, f))[top] for f in FIELDS)))
    print(f"{s['name']}: largest num_best {int(res.num_best[top[0]])}")
    for q, r in enumerate(top):
        want = inc.place_sample(*reads.entries(int(r)), want_best_vec=True)["best_j_vec"]
        assert got[q].tolist() == want.tolist(), (s["name"], int(r))


@pytest.mark.gpu
def test_shape_pipelined_call(shaped):
    """70 000 reads (the batch repeated) in four sub-batches, after a poison call (the same reads reversed): every
    result that of the unsplit call."""
    s = shaped
    mat, reads, res = s["mat"], s["reads"], s["res"]
    idx = np.resize(np.arange(reads.n_reads), 70_000)
    big = rk.take(reads, idx)
    mat.set_pipeline(4)
    try:
        mat.place_batch(rk.take(big, np.arange(big.n_reads)[::-1]))
        got = mat.place_batch(big)
    finally:
        mat.set_pipeline(0)
    assert_equal(got, res, f"{s['name']}: four sub-batches", idx=idx)
