"""The tile sweeps (sweep_kernels.hip: plain, dense and window table variants of sweep_tile, k_sweep_arena, the
finalize kernels) at their layout edges: every case of tests/sweep_cases.py through wepp_place_batch against the
oracle, bit for bit, every read of every batch.  tests/test_sweep_cases.py shows on the input's side that each case
sits on its edge; here one child process per group (WEPP_DEBUG_PLANS=1) shows that the device took the plan the
restated launch rule predicts -- T, ntiles, nchunks, bpc, NB, ncp, dense, ent_cap, key_cap of every `[plan]` line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sweep_cases as sc
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

GROUPS = {
    "tile_rule": [n for n in sc.CASES if n.startswith(("maxk_", "count_", "tile_"))],
    "plain": [n for n in sc.CASES if n.startswith("own_")],
    "dense": [n for n in sc.CASES if n.startswith("dense_")],
    "positions": [n for n in sc.CASES if n.startswith(("pos_a", "pos_b", "pos_e", "pos_f"))],
    "last_position": [n for n in sc.CASES if n.startswith(("pos_c", "pos_d"))],
    "blocks": [n for n in sc.CASES if n.startswith("heavy_")],
    "chunks": [n for n in sc.CASES if n.startswith("chunk_")],
    "finalize": [n for n in sc.CASES if n.startswith("finalize_")],
    "window": [n for n in sc.CASES if n.startswith("win_")],
    "arena": [n for n in sc.CASES if n.startswith("arena_")],
}


def test_every_case_has_a_group():
    assert sorted(n for g in GROUPS.values() for n in g) == sorted(sc.CASES)


class _Res:
    def __init__(self, d):
        self.score = np.array(d["score"], np.int32)
        self.best_bfs_j = np.array(d["best_bfs_j"], np.uint32)
        self.num_best = np.array(d["num_best"], np.uint32)
        self.flags = np.array(d["flags"], np.uint32)
        self.has_unique = (self.flags & 1).astype(np.uint8)


def run_group(names):
    """{(name, count): (result record, [plan] lines)} of one child process."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "sweep_edges_child.py")] + names,
                         env=dict(os.environ, WEPP_DEBUG_PLANS="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    recs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    plans, key = {}, None
    for l in out.stderr.splitlines():
        if l.startswith("[case]"):
            _, name, count = l.split()
            key = (name, int(count))
            plans[key] = []
        elif l.startswith("[plan]") and key is not None:
            plans[key].append(l)
    return {(r["name"], r["count"]): (r, plans[(r["name"], r["count"])]) for r in recs}


def want_of(oracle, case):
    """The oracle's answers for the whole batch of a case (prefixes are slices of it)."""
    ot = oracle.OracleTree(case.tree)
    if case.tree.n_nodes > 60000:
        # the 65 K-node trees: the incremental checker takes the batch, the faithful restatement a handful of reads
        want = ot.incremental().place_batch(case.reads, nthreads=os.cpu_count() or 1)
        few = ot.place_batch(case.reads.slice(0, min(5, case.reads.n_reads)), os.cpu_count() or 1)
        for k in ("score", "best_j", "num_best", "has_unique"):
            assert (want[k][:len(few)] == few[k]).all(), k
        return want
    return ot.place_batch(case.reads, os.cpu_count() or 1)


@pytest.mark.parametrize("group", sorted(g for g in GROUPS if GROUPS[g]))
def test_sweep_edges(oracle, group):
    names = GROUPS[group]
    got = run_group(names)
    assert sorted(got) == sorted((n, c) for n in names for c in sc.CASES[n]().counts)
    for name in names:
        case = sc.CASES[name]()
        want = want_of(oracle, case)
        for count in case.counts:
            rec, plans = got[(name, count)]
            ctx = "%s, %d reads" % (name, count)
            assert_same(_Res(rec), {k: np.asarray(want[k])[:count] for k in ("score", "best_j", "num_best", "has_unique")}, ctx)
            sc.check_device_plans(case, count, rec, [sc.parse_plan_line(l) for l in plans], ctx)
