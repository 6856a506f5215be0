"""wepp_place_batch's pipeline (place_batch.cpp): a host batch of 65 536 reads or more is cut into S sub-batches, sub-batch k
placed on the handle's lane k % 2, from one host thread or from two.  Every plan class goes through both lanes here --
whole-genome samples far from the tree among them, which k_seed hands to its second pass through a table of the lane
(seed_kernels.hip: SeedHeavy) -- and every result must be the unsplit call's.

Each configuration gets a fresh handle whose calls all have the same size, and a poison call first: the same reads in
reversed order, so that the handle's device result buffer holds another read's answer at every index and a result the
pipelined call never writes cannot pass."""
import os
import time

import numpy as np
import pytest

import read_kinds as rk
import wepp_amd as w

pytestmark = pytest.mark.gpu
FIELDS = ("best_bfs_j", "score", "num_best", "flags")
NTHREADS = min(16, os.cpu_count() or 1)
SEED_HEAVY_CAP = 128           # device_mat.hpp: samples one call (now: one sub-batch) hands to k_seed's second pass
BIG = 524_288                  # from here a call of the default split goes as two sub-batches when it has two launchers
KINDS = ("short", "nrich", "long", "hot", "empty", "genome", "far")


def new_mat(tree, **env):
    """A handle made with WEPP_SEED_CHUNK_BLOCKS=1 (a 120 K-node tree in > 1 500 chunks: far samples face levels of
    hundreds of chunks) and the given environment (read once, when the handle is created)."""
    env = {"WEPP_SEED_CHUNK_BLOCKS": "1", **env}
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


def sub_ranges(n, S):
    """the reads [lo, hi) of the S sub-batches of a call of n reads (read_check.hpp: sub_lo)"""
    return [(n * k // S, n * (k + 1) // S) for k in range(S)]


def assert_equal(got, want, ctx, idx=None):
    for f in FIELDS:
        a = np.asarray(getattr(got, f))
        b = np.asarray(getattr(want, f))
        if idx is not None:
            b = b[idx]
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{ctx}: {f} differs at {bad.size} reads, first {bad[:8].tolist()} (got {a[bad[:4]].tolist()}, want {b[bad[:4]].tolist()})"


def assert_checker(res, want, ctx):
    for name, got, exp in (("score", res.score, want["score"]), ("best_bfs_j", res.best_bfs_j, want["best_j"]),
                           ("num_best", res.num_best, want["num_best"]), ("has_unique", res.has_unique, want["has_unique"])):
        bad = np.flatnonzero(np.asarray(got) != np.asarray(exp))
        assert bad.size == 0, f"{ctx}: {name} differs at reads {bad[:10].tolist()}"


def place_after_poison(mat, reads):
    rev = rk.take(reads, np.arange(reads.n_reads)[::-1])
    mat.place_batch(rev)
    return mat.place_batch(reads)


@pytest.fixture(scope="module")
def lanes(oracle):
    """The tree, the shuffled mixed batch, the kind of every read, and the unsplit call's results and plans."""
    g = w.generate_tree(33, 120_000)
    rng = np.random.default_rng(2024)
    parts = {
        "short": g.reads(34, 56_000, p_substitution=0.003, p_n=0.02, p_iupac=0.1),       # walk8 / walk16 (N, IUPAC)
        "nrich": rk.concat([g.reads(35, 4000, p_n=0.10), g.reads(36, 2000, p_substitution=0.01, p_n=0.20)]),  # 17-32: sweeps of a crown
        "long": rk.long_reads(g, 37, 1600),                                               # > 32 entries: window plans
        "hot": rk.hot_position_reads(g.tree, rng, 2400),                                  # many events: waves, jobs
        "empty": rk.empty_reads(400),
        "genome": rk.genome_samples(g, 38, 600),                                          # seeded
        "far": rk.far_samples(rng, 400),                                                  # seeded, second pass
    }
    batch = rk.concat([parts[k] for k in KINDS])
    kind = np.concatenate([np.full(parts[k].n_reads, i) for i, k in enumerate(KINDS)])
    perm = np.random.default_rng(7).permutation(batch.n_reads)
    reads, kind = rk.take(batch, perm), kind[perm]
    assert reads.n_reads >= 65_536                     # (a pipelined call)

    m1 = new_mat(g.tree)
    m1.set_pipeline(1)
    whole = place_after_poison(m1, reads)
    m1.timing_reset()
    again = m1.place_batch(reads)
    assert_equal(again, whole, "unsplit call, twice")
    cls, _ = m1.last_plans(reads.n_reads)
    _, evaluated, _ = m1.last_seeds()
    m1.close()
    yield dict(g=g, reads=reads, kind=kind, whole=whole, cls=cls, evaluated=evaluated)
    g.close()


def test_batch_covers_every_class_in_every_sub_batch(lanes):
    """At S = 8 every sub-batch holds every plan class, and between 20 and 100 samples for the second pass (under the
    table's 128 per lane); at S = 2 more than 128 (the overflow stays with the first pass); the second pass ran."""
    cls, kind, n = lanes["cls"], lanes["kind"], lanes["reads"].n_reads
    far = kind == KINDS.index("far")
    assert (cls[far] == w.PLAN_SEED).all() and (cls[kind == KINDS.index("genome")] == w.PLAN_SEED).all()
    for lo, hi in sub_ranges(n, 8):
        c = np.bincount(cls[lo:hi], minlength=7)
        for p in (w.PLAN_WALK8, w.PLAN_WALK16, w.PLAN_SWEEP, w.PLAN_WIN, w.PLAN_SEED):
            assert c[p] >= 50, (lo, w.PLAN_NAMES[p], c.tolist())
        for p in (w.PLAN_WALKC8, w.PLAN_WALKC16):
            assert c[p] >= 20, (lo, w.PLAN_NAMES[p], c.tolist())
        assert 20 <= far[lo:hi].sum() <= 100, (lo, int(far[lo:hi].sum()))
        assert (kind[lo:hi] == KINDS.index("empty")).sum() > 0
    for lo, hi in sub_ranges(n, 2):
        assert far[lo:hi].sum() > SEED_HEAVY_CAP, (lo, int(far[lo:hi].sum()))
    # (the poison call leaves read n-1-i's answer at index i: for nearly every far sample another answer than its own --
    # in the score and num_best mostly, as most of them share one best node)
    stale = np.zeros(n, bool)
    for f in FIELDS:
        a = np.asarray(getattr(lanes["whole"], f))
        stale |= a[::-1] != a
    assert stale[far].mean() > 0.9, stale[far].mean()
    # (the same proxy as test_seed_gpu.py: the far samples do face levels of 256 chunks or more)
    assert lanes["evaluated"] > 256 * int(far.sum()), (lanes["evaluated"], int(far.sum()))


def test_unsplit_call_vs_checker_oracle_and_one_pass(lanes, oracle):
    """The unsplit call against the incremental checker on every read, the faithful oracle on six (one of each kind
    but the empty), and a handle without the seed kernel's second pass on every read."""
    g, reads, kind, whole = lanes["g"], lanes["reads"], lanes["kind"], lanes["whole"]
    ot = oracle.OracleTree(g.tree)
    t0 = time.perf_counter()
    want = ot.incremental().place_batch(reads, nthreads=NTHREADS)
    print(f"checker: {reads.n_reads} reads in {time.perf_counter() - t0:.2f} s")
    assert_checker(whole, want, "unsplit vs the incremental checker")
    six = np.array([int(np.flatnonzero(kind == KINDS.index(k))[0]) for k in KINDS if k != "empty"])
    few = rk.take(reads, six)
    sub = w.PlacementResult(*(np.asarray(getattr(whole, f))[six] for f in FIELDS))
    assert_checker(sub, ot.place_batch(few, NTHREADS), "unsplit vs the faithful oracle")
    m0 = new_mat(g.tree, WEPP_SEED_HEAVY="0")
    m0.set_pipeline(1)
    assert_equal(place_after_poison(m0, reads), whole, "second pass off")
    m0.close()


@pytest.mark.parametrize("host_threads", [2, 4])
@pytest.mark.parametrize("S", [2, 3, 4, 8])
def test_pipelined_call_equals_unsplit(lanes, S, host_threads):
    """S sub-batches on the two lanes: WEPP_HOST_THREADS=2 (one host worker: one launcher, the lanes still alternate
    and their kernels may overlap on the device) and 4 (two launchers)."""
    mat = new_mat(lanes["g"].tree, WEPP_HOST_THREADS=host_threads)
    mat.set_pipeline(S)
    got = place_after_poison(mat, lanes["reads"])
    mat.close()
    assert_equal(got, lanes["whole"], f"S={S}, WEPP_HOST_THREADS={host_threads}")


def test_default_split_of_a_large_call(lanes):
    """S = 0 (the product's choice) on 524 288 reads with two launchers: two sub-batches, one per lane, each with far
    more samples for the second pass than its table holds."""
    reads = lanes["reads"]
    idx = np.resize(np.arange(reads.n_reads), BIG)
    big = rk.take(reads, idx)
    mat = new_mat(lanes["g"].tree, WEPP_HOST_THREADS=4)
    mat.set_pipeline(0)
    got = place_after_poison(mat, big)
    mat.close()
    assert_equal(got, lanes["whole"], "default split, 524 288 reads", idx=idx)
