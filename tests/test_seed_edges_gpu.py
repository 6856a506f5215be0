"""k_seed (wepp_amd/csrc/seed_kernels.hip) at its internal thresholds: every case of tests/seed_cases.py through
Mat.place_batch against the faithful oracle, bit for bit -- score, best_bfs_j, num_best, has_unique of every sample.
tests/test_seed_cases.py shows on the input's side that each case sits on its edge; here the device must have SEEDED
the samples the case names (Mat.last_plans: a case that passes through the tile sweeps proves nothing), must report
the `[plan] seed` line the case predicts (count, maxk, chunks, the LDS request recomputed from seed_lds_bytes's
formula, the words' room = maxk rounded up to 64), must give the same answers with the seeds off, and must have
evaluated at least the chunks the model says it must and no more than it may (Mat.last_seeds)."""
import os

import numpy as np
import pytest

import seed_cases as sc
import seed_model as sdm
import wepp_amd as w
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
FIELDS = ("score", "best_j", "num_best", "has_unique")


@pytest.fixture(scope="module")
def handles():
    """One device handle per (tree, environment), shared by the cases on that tree; walks off: a read that can walk
    never reaches the sweeps' plans."""
    cache = {}

    def get(case, **extra):
        env = dict(case.env, WEPP_DEBUG_PLANS="1", WEPP_SEED_HEAVY=None)
        env.update(extra)
        key = (case.key, tuple(sorted((k, str(v)) for k, v in env.items())))
        if key not in cache:
            with sc.environment(env):
                mat = w.Mat(case.tree)
            mat.set_use_walk(False)
            assert mat.stats.seed_chunks == case.model.nch and mat.stats.seed_chunk_blocks == case.stride
            cache[key] = mat
        return cache[key]
    yield get
    for mat in cache.values():
        mat.close()


_WANT = {}


def want_of(oracle, case):
    if case.name not in _WANT:
        ot = oracle.OracleTree(case.tree)
        _WANT[case.name] = ot.place_batch(case.reads, min(8, os.cpu_count() or 1))
        ot.close()
    return _WANT[case.name]


def place(mat, reads, capfd):
    """(results, plan class per sample, (samples seeded, chunks evaluated, chunks in all), the `[plan] seed` lines)"""
    mat.timing_reset()
    capfd.readouterr()
    res = mat.place_batch(reads)
    err = capfd.readouterr().err
    cls, _ = mat.last_plans(reads.n_reads)
    lines = []
    for l in err.splitlines():
        if l.startswith("[plan] seed "):
            lines.append({kv.split("=")[0]: int(kv.split("=")[1]) for kv in l.split()[2:]})
    return res, np.asarray(cls), mat.last_seeds(), lines


def check_seeded_run(case, oracle, count, got, ctx):
    res, cls, (samples, evaluated, total), lines = got
    names = case.names[:count]
    print(ctx, "plans", cls.tolist()[:12], "seeds", (samples, evaluated, total), "lines", lines)
    assert [n for n, c in zip(names, cls) if c == sc.PLAN_SEED] == [n for n in names if n in case.seeded], (ctx, cls.tolist())
    seeded = [n for n in names if n in case.seeded]
    maxk = max(len(case.samples[n]) for n in seeded)
    cap = (maxk + 63) & ~63                                   # the words' room in LDS: the batch maximum rounded up to 64
    m = case.model
    assert lines == [dict(count=len(seeded), maxk=maxk, chunks=m.nch, lds=sdm.seed_lds_bytes(m.bm_words, cap, m.nch))], (ctx, lines)
    assert samples == len(seeded) and total == samples * m.nch, ctx
    lo, hi = sc.evaluated_bounds(case, oracle, count)
    print(ctx, "evaluated", evaluated, "must", lo, "may", hi)
    if case.over_max_hard():
        # more than SEED_MAX_HARD hard entries inside the tree: the kernel counts an arbitrary 255 of them (the order
        # of its atomics), so which chunks it must look at is not determined -- only that there are no more than all
        assert 1 <= evaluated <= total, ctx
    else:
        assert lo <= evaluated <= hi, (ctx, lo, evaluated, hi)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_seed_edges(oracle, handles, capfd, name):
    case = sc.CASES[name]()
    want_all = want_of(oracle, case)
    mat = handles(case)
    for count in case.counts:
        reads = case.reads.slice(0, count)
        want = {k: np.asarray(want_all[k])[:count] for k in FIELDS}
        ctx = "%s, %d samples" % (name, count)
        got = place(mat, reads, capfd)
        assert_same(got[0], want, ctx + " vs the oracle")
        check_seeded_run(case, oracle, count, got, ctx)
        if case.deferral:
            # the table of the second pass is cleared between calls: the same batch again on the same handle
            again = place(mat, reads, capfd)
            assert_same(again[0], want, ctx + ", second call")
            check_seeded_run(case, oracle, count, again, ctx + ", second call")
            # one pass only (a handle of its own): every sample's workgroup evaluates all it must itself
            one = handles(case, WEPP_SEED_HEAVY="0")
            got1 = place(one, reads, capfd)
            assert_same(got1[0], want, ctx + ", one pass")
            check_seeded_run(case, oracle, count, got1, ctx + ", one pass")
        # the same samples through the tile sweeps
        mat.set_use_seeds(False)
        try:
            res, cls, _, lines = place(mat, reads, capfd)
        finally:
            mat.set_use_seeds(True)
        assert not (cls == sc.PLAN_SEED).any() and lines == [], ctx
        assert_same(res, want, ctx + ", seeds off")
