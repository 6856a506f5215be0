"""A placement call whose partials outgrow what the handle has (capi.cpp: place_device, handle.hpp: PlaceLane).

A lane owns two grow-only device blocks.  `ws` holds the regions sized by the number of reads alone; it is grown before
k_route and never moves during a call.  `part` holds the partials of the sweep plans, 12 bytes per (chunk, read), sized
only when the routing counters are back; it is grown behind the planner, before anything of the call touches it.  So
a call whose partials do not fit routes once, like every other call: WEPP_DEBUG_PLANS=1 prints one "[route]" and one
"[step]" line per call.  (While both shared one block, such a call freed the block under its own routing, allocated a
larger one and routed a second time: two "[step]" lines.)

The tree has 2.5 M nodes: its tree-wide stream is ~18 MB, which a sweep of reads this long cuts into 32 chunks.  Two
batches:
  A  3 000 plain walkers: nothing reads the grouped list, no partials;
  X  the same walkers and 320 000 reads of 20 - 30 N entries (300 distinct ones, repeated), which can only sweep the
     tree-wide stream: 320 000 * 32 * 12 bytes = 123 MB of partials behind 323 000 reads -- more than the half of the
     fixed regions plus 36 bytes per read (~45 MB) that the single block of old had to spare after its first growth.
     Seen once with the library of the commit before the split: the first call of a fresh handle on X printed one
     "[route]" and TWO "[step]" lines, and "[plan] sweep t=13 count=320000 ... nchunks=32".
The incremental checker is the reference, computed once for the distinct reads and indexed."""
import os
import re

import numpy as np
import pytest

import read_kinds as rk
import wepp_amd as w
from test_lazy_lists import LISTS_LINE, assert_checker, assert_equal, n_only_reads

pytestmark = pytest.mark.gpu
NTHREADS = min(16, os.cpu_count() or 1)
N_NODES = 2_500_000
N_WALKERS, N_SWEEPERS, N_DISTINCT_SWEEPERS = 3000, 320_000, 300
STEP_LINE = re.compile(r"^\[step\] ", re.M)
SWEEP_PLAN = re.compile(r"^\[plan\] sweep t=(\d+) count=(\d+) .* nchunks=(\d+) ", re.M)


def new_mat(world):
    """a handle on the shared flat image that prints its routing, one device call per place_batch"""
    old = os.environ.get("WEPP_DEBUG_PLANS")
    os.environ["WEPP_DEBUG_PLANS"] = "1"
    try:
        mat = w.Mat(world["g"].tree, flat=world["flat"])
    finally:
        if old is None:
            os.environ.pop("WEPP_DEBUG_PLANS", None)
        else:
            os.environ["WEPP_DEBUG_PLANS"] = old
    mat.set_pipeline(1)
    return mat


@pytest.fixture(scope="module")
def world(oracle):
    g = w.generate_tree(33, N_NODES)
    flat = w.FlatView(g.tree)
    rng = np.random.default_rng(77)
    pool = g.reads(34, 8000, p_substitution=0.003, p_n=0.02, p_iupac=0.1)
    probe = w.Mat(g.tree, flat=flat)
    probe.place_batch(pool)
    cls, _ = probe.last_plans(pool.n_reads)
    probe.close()
    plain = np.flatnonzero(cls == w.PLAN_WALK8)[:N_WALKERS]
    assert plain.size == N_WALKERS, np.bincount(cls, minlength=7).tolist()
    # U = the distinct reads, the walkers first; the checker places each once
    U = rk.concat([rk.take(pool, plain), n_only_reads(rng, N_DISTINCT_SWEEPERS)])
    want_u = oracle.OracleTree(g.tree).incremental().place_batch(U, nthreads=NTHREADS)
    a_idx = np.random.default_rng(5).permutation(N_WALKERS)
    x_idx = np.concatenate([np.arange(N_WALKERS), np.resize(np.arange(N_WALKERS, U.n_reads), N_SWEEPERS)])
    x_idx = np.random.default_rng(6).permutation(x_idx)
    yield dict(g=g, flat=flat, A=rk.take(U, a_idx), X=rk.take(U, x_idx), want={"A": want_u[a_idx], "X": want_u[x_idx]})
    flat.close()
    g.close()


def place(mat, world, x, mode, capfd, ctx):
    """one call of batch x: one [route] and one [step] line, k_scatter as `mode` says, X's sweep plan; returns the result"""
    res = mat.place_batch(world[x])
    err = capfd.readouterr().err
    print(err, end="")
    steps = STEP_LINE.findall(err)
    routes = [ln for ln in err.splitlines() if ln.startswith("[route] ")]
    assert len(routes) == 1 and len(steps) == 1, f"{ctx}: {len(routes)} [route] and {len(steps)} [step] lines"
    assert LISTS_LINE.findall(err) == [(mode, "0" if mode == "none" else "1")], (ctx, mode, err)
    if x == "A":
        assert not SWEEP_PLAN.findall(err), (ctx, err)
    else:
        # what makes X outgrow the handle: every sweeper in ONE plan of the tree-wide stream, cut into 16 chunks or more
        plans = [(int(t), int(c), int(k)) for t, c, k in SWEEP_PLAN.findall(err)]
        assert len(plans) == 1 and plans[0][1] == N_SWEEPERS and plans[0][2] >= 16, (ctx, plans)
        assert plans[0][0] + 1 == world["flat"].n_streams, (ctx, plans)
    return res


def run_sequence(world, capfd, order, modes):
    """The batches `order` on one fresh handle.  modes: k_scatter of every call -- A alone needs no list ("none"); X has
    consumers the hint did not expect ("late"); an A behind an X pays the blind launch the hint of X asked for, and that
    keeps the next X from setting the hint again (test_lazy_lists.py)."""
    mat = new_mat(world)
    try:
        capfd.readouterr()
        got = {}
        for i, x in enumerate(order):
            res = place(mat, world, x, modes[i], capfd, f"call {i} ({x}) of {order}")
            if x in got:
                assert_equal(res, got[x], f"call {i} ({x}) of {order} against the first {x}")
            else:
                assert_checker(res, world["want"][x], f"call {i} ({x}) of {order}")
                got[x] = res
    finally:
        mat.close()


def test_fresh_handle_outgrows_its_partials(world, capfd):
    """X on a fresh handle, then A, X and A again: every call routes once, X equals the checker and itself, A too."""
    run_sequence(world, capfd, "XAXA", ("late", "blind", "late", "none"))


def test_partials_grow_on_a_handle_that_has_run(world, capfd):
    """A first, X second, then both again: the block of the partials grows on a handle whose fixed regions are in use."""
    run_sequence(world, capfd, "AXAX", ("none", "late", "blind", "late"))
