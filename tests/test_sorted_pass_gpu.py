"""The sorted pass of a read with more than 64 events (place_dev.hpp: sorted_build, sorted_query) on the GPU, bit for
bit against the incremental checker.

The tree is small and its genome short -- 6 000 nodes over 400 positions, 1 - 255 mutations per mutated position, 11 at
the median --, and a read lists 9 - 16 positions drawn uniformly from the 400 MUTATED positions (position 0 carries no
mutation and is left out: drawn from all 401, fewer reads reach 65 events).  Of 400 reads (seed 3) 326 have 65 - 256
events in the whole-tree stream, 263 of them more than 128, and most of them several entries on one node, a shared
subtree end and an entry node at another entry's end -- the ties the sort must get right, which the 60 000-node tree of
test_fused_step.py rarely produces.  A hub tree and a deep one of the same size follow (long runs of leaves with empty
stretches between them, long chains of equal ends), then a batch whose reads of 256 / 65 / 129 / 193 events outnumber
the wave-role workgroups of k_step, so that a workgroup takes a small read right after a large one.

How many reads of a batch the sorted pass gets is not guessed: the CPU model of the routing (sweep_model.TieredModel)
names every read's stream, walk_model counts its events there, and k_route's own counter of the class with more than
64 events must equal the model's count on a fresh handle."""
import os

import numpy as np
import pytest

import read_kinds as rk
import sweep_model as sm
import walk_model as wm
import wepp_amd as w
from test_fused_step import assert_checker, assert_equal, entry, ladder_reads, position_table, route_counts, wave_role_workgroups
from wepp_amd import Reads

NTHREADS = min(16, os.cpu_count() or 1)
TREE = dict(genome_len=400, p_ambiguous=0.02, p_masked_node=0.003, root_mutations=1)


def draw_reads(tree, seed, n):
    """n reads of 9 - 16 entries at distinct uniformly drawn positions, and their events in the whole-tree stream"""
    counts, ref = position_table(tree)
    mutated = np.flatnonzero(counts > 0)
    rng = np.random.default_rng(seed)
    samples, totals = [], []
    for _ in range(n):
        pos = np.sort(rng.choice(mutated, size=int(rng.integers(9, 17)), replace=False))
        samples.append([entry(rng, p, ref) for p in pos])
        totals.append(int(counts[pos].sum()))
    return samples, np.array(totals)


def routed_events(tree, samples):
    """every read's events in the stream the routing model sends it to"""
    fv = w.FlatView(tree)
    tiers, models, ev = sm.TieredModel(fv), {}, []
    for S in samples:
        st = tiers.route(S)
        m = models.get(st) or models.setdefault(st, wm.WalkModel(fv, st))
        ev.append(m.events_of(S))
    fv.close()
    return np.array(ev)


def check_batch(g, inc, reads, monkeypatch, capfd, ctx, variants=True):
    """the batch on a fresh handle against the checker; what k_route made of it; the same arrays on a second call, from
    the launch of its own (k_walk_wave: four waves a workgroup) and from a handle that goes by jobs"""
    want = inc.place_batch(reads, nthreads=NTHREADS)
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    mat = w.Mat(g.tree)
    try:
        res = mat.place_batch(reads)
        c = route_counts(capfd)
        cls, _ = mat.last_plans(reads.n_reads)
        print(ctx, c, np.bincount(cls, minlength=7).tolist())
        assert_checker(res, want, ctx)
        assert_equal(mat.place_batch(reads), res, f"{ctx}: second call")
    finally:
        mat.close()
    if variants:
        for env, name in (({"WEPP_STEP_UNFUSED": "1"}, "a launch of its own"),
                          ({"WEPP_WW_BLOCK_MAX_SMALL": "0", "WEPP_WW_BLOCK_MAX_BIG": "0"}, "by jobs")):
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                m2 = w.Mat(g.tree)           # (the switches are read when the handle is created)
            try:
                assert_equal(m2.place_batch(reads), res, f"{ctx}: {name}")
                c2 = route_counts(capfd)
                assert (c2["wave_big"] == 0) == (name == "by jobs"), (name, c2)
            finally:
                m2.close()
    return c, cls


@pytest.mark.gpu
def test_reads_of_9_to_16_entries_with_many_events(oracle, monkeypatch, capfd):
    g = w.generate_tree(61, 6000, **TREE)
    try:
        counts, _ = position_table(g.tree)
        counts = counts[counts > 0]
        assert (int(counts.min()), int(counts.max()), int(np.median(counts))) == (1, 255, 11), (counts.min(), counts.max(), np.median(counts))
        samples, totals = draw_reads(g.tree, 3, 400)
        assert (((totals > 64) & (totals <= 256)).sum(), ((totals > 128) & (totals <= 256)).sum()) == (326, 263)
        ev = routed_events(g.tree, samples)
        assert (ev == totals).all()                # (every read of this batch is routed to the whole-tree stream)
        reads = Reads.from_lists(samples)
        c, cls = check_batch(g, oracle.OracleTree(g.tree).incremental(), reads, monkeypatch, capfd, "9 - 16 entries")
        # every read of the batch has 9 - 16 entries, and all 326 with 65 - 256 events went to the sorted pass; the 74 with
        # more are cut into jobs
        assert (c["reads"], c["wave_big"], c["jobs16"]) == (400, 326, 74), c
        assert (cls == w.PLAN_WALKC16).sum() == 400, np.bincount(cls).tolist()
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [dict(p_hub=0.5), dict(depth_choices=3)], ids=["hub", "deep"])
def test_hub_and_deep_trees(oracle, monkeypatch, capfd, shape):
    g = w.generate_tree(61, 6000, **TREE, **shape)
    try:
        samples, totals = draw_reads(g.tree, 4, 300)
        assert ((totals > 64) & (totals <= 256)).sum() >= 100, np.sort(totals).tolist()
        ev = routed_events(g.tree, samples)
        big = int(((ev > 64) & (ev <= 256)).sum())
        # the hub tree's reads all walk the whole-tree stream (every read in range is a read of the sorted pass); the deep
        # tree's are routed to smaller streams, where most of them keep 64 events or fewer: a handful is left for it
        in_range = int(((totals > 64) & (totals <= 256)).sum())
        assert big == in_range if "p_hub" in shape else 0 < big < 20, (big, in_range, np.sort(ev).tolist())
        c, _ = check_batch(g, oracle.OracleTree(g.tree).incremental(), Reads.from_lists(samples), monkeypatch, capfd, str(shape), variants=False)
        assert c["wave_big"] == big, (c, big)
    finally:
        g.close()


@pytest.mark.gpu
def test_small_read_behind_a_large_one_in_the_same_workgroup(oracle, monkeypatch, capfd):
    """~100 distinct reads whose events in the tree go 256, 65, 129, 193, 256, ... repeated to more than twice the
    wave-role workgroups: every workgroup takes several in a row and must not see the LDS of the read before"""
    g = w.generate_tree(61, 6000, **TREE)
    try:
        wave_wgs = wave_role_workgroups()
        samples, total_of = ladder_reads(g.tree, np.resize(np.array([256, 65, 129, 193]), 100), per_total=1, seed=7)
        assert total_of.tolist()[:5] == [256, 65, 129, 193, 256]
        distinct = Reads.from_lists(samples)
        inc = oracle.OracleTree(g.tree).incremental()
        want100 = inc.place_batch(distinct, nthreads=NTHREADS)
        idx = np.resize(np.arange(distinct.n_reads), 2 * wave_wgs + 3)
        reads = rk.take(distinct, idx)
        want = want100[idx]
        monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
        for env in ({}, {"WEPP_STEP_UNFUSED": "1"}):
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                mat = w.Mat(g.tree)
            try:
                res = mat.place_batch(reads)
                c = route_counts(capfd)
                print(env, c)
                assert_checker(res, want, f"in turn {env}")
                assert c["wave_big"] > wave_wgs, (c, wave_wgs)
            finally:
                mat.close()
    finally:
        g.close()
