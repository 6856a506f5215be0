"""The routing counters of a placement call reach the host by k_step's report (walk_kernels.hip: the first wave of the
launch stores them into the lane's block of host memory and the call's sequence number behind them; capi.cpp polls that
word) instead of a copy on the plan stream.  WEPP_INFO_COPY=1 keeps the copy: every case here runs on a handle of each
kind, results go into device arrays filled with 0x7FFFFFFF, and the four arrays and the "[route]" and "[lists]" lines
(WEPP_DEBUG_PLANS=1) must be the same, word for word.  "[info]" says which way a call's counters came.

Two small worlds of the existing tests: the 30 000-node tree of tests/test_route_tables_gpu.py with its per-read batch
(resolved reads, walkers of both classes, wave reads of both sizes) and the 60 000-node tree of
tests/test_lazy_lists.py with reads of the consumers (sweeps, window tiles, seeded samples), whose launches need the
grouped read list: k_scatter then goes late, behind the report, and the plan stream is joined."""
import re
import threading
import time

import numpy as np
import pytest

import read_kinds as rk
import wepp_amd as w
from test_lazy_lists import FIELDS, consumer_masks, n_only_reads, new_mat
from test_route_tables_gpu import FILL, Router, kinds, make_tree, many_event_reads
from test_step_groups import BY_JOBS, GROUPS_OFF, WIDE
from wepp_amd import Reads

pytestmark = pytest.mark.gpu
INFO_LINE = re.compile(r"\[info\] counters by (report|copy), lane (\d+), sequence (\d+)")
ROUTE_FIELDS = re.compile(r"\d+")
COPY = {"WEPP_INFO_COPY": "1"}


class DevBatch:
    """A batch on the device; run() places it into four arrays of its own, filled with FILL, without synchronising."""

    def __init__(self, reads):
        import torch
        self.torch, self.dev, self.reads = torch, torch.device("cuda", 0), reads
        self.d_off = torch.from_numpy(reads.read_off.astype(np.int32)).to(self.dev)
        rw = reads.read_word if reads.read_word.size else np.zeros(1, np.uint32)
        self.d_word = torch.from_numpy(rw.astype(np.int32)).to(self.dev)

    def run(self, mat, stream=0):
        outs = [self.torch.full((self.reads.n_reads,), FILL, dtype=self.torch.int32, device=self.dev) for _ in range(4)]
        mat.place_batch_device(self.d_off.data_ptr(), self.d_word.data_ptr(), self.reads.n_reads, int(self.reads.read_off[-1]),
                               *[o.data_ptr() for o in outs], stream)
        return outs


def arrays(outs):
    return [o.cpu().numpy().view(np.uint32) for o in outs]


def assert_same(got, want, ctx):
    for f, a, b in zip(FIELDS, got, want):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{ctx}: {f} differs at {bad.size} reads, first {bad[:8].tolist()} (got {a[bad[:4]].tolist()}, want {b[bad[:4]].tolist()})"


def lines(capfd):
    """the "[route]" lines, the "[lists]" lines and the (way, lane, sequence) of the "[info]" lines printed since the last look"""
    err = capfd.readouterr().err.splitlines()
    info = [(m.group(1), int(m.group(2)), int(m.group(3))) for m in map(INFO_LINE.match, err) if m]
    return [l for l in err if l.startswith("[route]")], [l for l in err if l.startswith("[lists]")], info


def one_call(tree, batch, env, capfd):
    """the batch placed by one call on a fresh handle: arrays, "[route]", "[lists]", "[info]" of the call"""
    import torch
    mat = new_mat(tree, **env)
    try:
        lines(capfd)
        outs = batch.run(mat)
        torch.cuda.synchronize()
        return (arrays(outs),) + lines(capfd)
    finally:
        mat.close()


def report_against_copy(tree, batch, capfd, ctx, **env):
    """one call by report and one by copy; returns the report call's "[route]" and "[lists]" line"""
    got, route, lists, info = one_call(tree, batch, env, capfd)
    want, route_c, lists_c, info_c = one_call(tree, batch, {**env, **COPY}, capfd)
    assert info == [("report", 0, 1)] and info_c == [("copy", 0, 0)], (ctx, info, info_c)
    assert len(route) == 1 and len(lists) == 1 and route == route_c and lists == lists_c, (ctx, route, route_c, lists, lists_c)
    assert_same(got, want, ctx)
    assert all((a != FILL).all() for a in got[1:3]), f"{ctx}: a read kept the fill value"
    return route[0], lists[0]


def route_numbers(line):
    return [int(x) for x in ROUTE_FIELDS.findall(line.replace("9 - 16", ""))]


@pytest.fixture(scope="module")
def rworld():
    """the tree of tests/test_route_tables_gpu.py, its per-read batch and its reads with many events, in one batch"""
    g = make_tree()
    fv = w.FlatView(g.tree)
    by_kind = kinds(g.tree, Router(fv), 11)
    reads = Reads.from_lists([S for v in by_kind.values() for S in v])
    many = many_event_reads(g.tree, None, 12, 3000)
    fv.close()
    mixed = rk.concat([reads, many])
    yield dict(g=g, mixed=mixed, dev=DevBatch(mixed))
    g.close()


@pytest.fixture(scope="module")
def lworld():
    """the tree of tests/test_lazy_lists.py; A: reads k_route, the walkers and the wave role place; B: A and reads of the
    consumers; C: reads without an entry, which k_route resolves all"""
    g = w.generate_tree(33, 60_000)
    rng = np.random.default_rng(78)
    A = rk.concat([g.reads(34, 3000, p_substitution=0.003, p_n=0.02, p_iupac=0.1), rk.hot_position_reads(g.tree, rng, 300, hot=400, k_lo=2, k_hi=6)])
    B = rk.concat([A, n_only_reads(rng, 200), rk.long_reads(g, 37, 400), rk.genome_samples(g, 38, 60), rk.far_samples(rng, 40)])
    B = rk.take(B, np.random.default_rng(6).permutation(B.n_reads))
    C = rk.empty_reads(500)
    yield dict(g=g, A=A, B=B, C=C, dev={x: DevBatch(r) for x, r in (("A", A), ("B", B), ("C", C))})
    g.close()


def test_mixed_batch(rworld, capfd):
    """(a) resolved reads, walkers of both classes, wave reads of both sizes"""
    route, lists = report_against_copy(rworld["g"].tree, rworld["dev"], capfd, "mixed batch")
    v = route_numbers(route)     # reads, resolved, walk8, walk16, wave small, wave big, ...
    # (a routing block hands its few walkers of 9 - 16 entries to the wave role: they are counted there or here)
    assert v[0] == rworld["mixed"].n_reads and v[1] > 0 and v[2] > 0 and v[3] + v[6] > 0 and v[4] > 0 and v[5] > 0, route


def test_consumers_launch_late_behind_the_report(lworld, capfd):
    """(b) sweeps, window tiles and seeded samples: k_scatter goes late and the plan stream is joined"""
    tree = lworld["g"].tree
    _, lists = report_against_copy(tree, lworld["dev"]["B"], capfd, "consumers")
    assert lists == "[lists] scatter=late plan stream joined=1", lists
    mat = new_mat(tree)
    try:
        mat.place_batch(lworld["B"])
        cls, st = mat.last_plans(lworld["B"].n_reads)
        masks = consumer_masks(cls, st)
        assert all(masks[n].sum() > 0 for n in ("sweep", "window", "seed")), {n: int(m.sum()) for n, m in masks.items()}
    finally:
        mat.close()
    # ... and blind, behind a call that had consumers: the plan stream forks in front of the poll
    mat, cp = new_mat(tree), new_mat(tree, **COPY)
    try:
        import torch
        lines(capfd)
        for i in range(3):
            got, want = lworld["dev"]["B"].run(mat), lworld["dev"]["B"].run(cp)
            torch.cuda.synchronize()
            assert_same(arrays(got), arrays(want), f"consumers, call {i}")
        route, lists, info = lines(capfd)
        assert route[0::2] == route[1::2] and lists[0::2] == lists[1::2], (route, lists)
        assert [l.split()[1] for l in lists[0::2]] == ["scatter=late", "scatter=blind", "scatter=blind"], lists
        assert info[0::2] == [("report", 0, i + 1) for i in range(3)], info
    finally:
        mat.close()
        cp.close()


def test_batch_k_route_resolves_entirely(lworld, capfd):
    """(c) both lists of k_step are empty: the report still arrives"""
    route, lists = report_against_copy(lworld["g"].tree, lworld["dev"]["C"], capfd, "all resolved")
    assert route_numbers(route)[:6] == [500, 500, 0, 0, 0, 0] and lists == "[lists] scatter=none plan stream joined=0", (route, lists)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_few_reads(rworld, capfd, n):
    """(d) fewer reads than a workgroup of k_step holds, and one more than a multiple"""
    idx = np.arange(rworld["mixed"].n_reads)[::11][:n]
    assert idx.size == n
    report_against_copy(rworld["g"].tree, DevBatch(rk.take(rworld["mixed"], idx)), capfd, f"{n} reads")


@pytest.mark.parametrize("env", [GROUPS_OFF, WIDE, BY_JOBS], ids=["lane = read", "groups of 16", "by jobs"])
def test_other_forms_of_k_step(rworld, capfd, env):
    """(e) k_step<0>, k_step<16> and a handle that cuts the reads with many events into jobs"""
    report_against_copy(rworld["g"].tree, rworld["dev"], capfd, str(env), **env)


def back_to_back(tree, batches, order, env, capfd):
    """the calls `order` on one handle and one stream, no synchronisation between them; returns arrays per call and lines"""
    import torch
    mat = new_mat(tree, **env)
    try:
        stream = torch.cuda.Stream()
        # (a warm-up call of each batch: the workspace has its final size, so no call below synchronises to regrow it)
        with torch.cuda.stream(stream):
            for x in sorted(set(order)):
                batches[x].run(mat, stream.cuda_stream)
        stream.synchronize()
        lines(capfd)
        with torch.cuda.stream(stream):
            outs = [batches[x].run(mat, stream.cuda_stream) for x in order]
        stream.synchronize()
        return ([arrays(o) for o in outs],) + lines(capfd)
    finally:
        mat.close()


def check_no_stale_report(tree, batches, order, capfd, ctx):
    got, route, lists, info = back_to_back(tree, batches, order, {}, capfd)
    want, route_c, lists_c, info_c = back_to_back(tree, batches, order, COPY, capfd)
    n_warm = len(set(order))
    assert [i[0] for i in info] == ["report"] * len(order) and [i[0] for i in info_c] == ["copy"] * len(order), (info, info_c)
    assert [i[2] for i in info] == list(range(n_warm + 1, n_warm + len(order) + 1)), info       # (a lane's sequence numbers rise by one a call)
    own = {}
    for x in set(order):            # (what k_route makes of each batch: the same in every call, by either way)
        own[x] = {r for r, y in zip(route_c, order) if y == x}
        assert len(own[x]) == 1, (ctx, x, own[x])
    assert len(route) == len(order) and len(lists) == len(order)
    assert len({frozenset(v) for v in own.values()}) == len(own), (ctx, own)
    for i, x in enumerate(order):
        assert route[i] in own[x], f"{ctx}: call {i} ({x}) printed the counters {route[i]!r}, its batch's are {own[x]}"
    assert lists == lists_c, (ctx, lists, lists_c)
    for i, x in enumerate(order):
        assert_same(got[i], want[i], f"{ctx}: call {i} ({x})")
    return own


def test_a_stale_report_shows(rworld, lworld, capfd):
    """40 calls back to back, alternating two batches: every call prints the counters of its own batch, and the
    "[lists]" sequence -- fed by the hints, which are fed by the counters -- is the copy handle's.  First two batches of
    the walkers' tree that differ in every counter they fill, then the consumers' batch and one without consumers in
    turn: calls with and without work on the plan stream."""
    mixed = rworld["mixed"]
    part = rk.take(mixed, np.concatenate([np.arange(0, mixed.n_reads - 3000, 3), np.arange(mixed.n_reads - 3000, mixed.n_reads, 2)]))
    own = check_no_stale_report(rworld["g"].tree, {"X": rworld["dev"], "Y": DevBatch(part)}, "XY" * 20, capfd, "two mixed batches")
    vx, vy = route_numbers(own["X"].pop()), route_numbers(own["Y"].pop())
    print("counters of the two batches:", vx, vy)
    filled = [i for i in range(11) if vx[i] or vy[i]]        # (the last two fields are flags, not counts)
    assert len(filled) >= 6 and all(vx[i] != vy[i] for i in filled), (vx, vy)      # (every counter either batch fills differs)
    check_no_stale_report(lworld["g"].tree, lworld["dev"], "BA" * 20, capfd, "with and without consumers")


def test_two_lanes_of_a_pipelined_call(lworld):
    """wepp_place_batch in two sub-batches, a launch thread and a lane each (a report block and a sequence of its own),
    against one call: the first half holds no consumer, the second does"""
    A, B = lworld["A"], lworld["B"]
    both = rk.concat([rk.take(A, np.resize(np.arange(A.n_reads), 66_000)), B])
    assert both.n_reads >= 65_536          # (a pipelined call)
    whole, split = new_mat(lworld["g"].tree), new_mat(lworld["g"].tree, WEPP_PIPE_SUBBATCHES="2")
    try:
        whole.set_pipeline(1)
        want = whole.place_batch(both)
        for i in range(2):
            got = split.place_batch(both)
            assert_same([np.asarray(getattr(got, f)).view(np.uint32) for f in FIELDS], [np.asarray(getattr(want, f)).view(np.uint32) for f in FIELDS],
                        f"two sub-batches, call {i}")
    finally:
        whole.close()
        split.close()


def test_two_handles_on_two_threads(lworld):
    """two handles, a host thread each, ten calls each, A and B in turn: the arrays a handle gives alone"""
    tree = lworld["g"].tree
    mats = [new_mat(tree), new_mat(tree)]
    try:
        for m in mats:
            m.set_pipeline(1)
        alone = [{x: m.place_batch(lworld[x]) for x in "AB"} for m in mats]
        order = ["ABABABABAB", "BABABABABA"]
        got, errors = [[], []], []

        def work(k):
            try:
                for x in order[k]:
                    got[k].append(mats[k].place_batch(lworld[x]))
            except Exception as e:      # (reported below, on the main thread)
                errors.append((k, repr(e)))

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k in range(2):
            assert len(got[k]) == 10
            for i, x in enumerate(order[k]):
                assert_same([np.asarray(getattr(got[k][i], f)).view(np.uint32) for f in FIELDS],
                            [np.asarray(getattr(alone[k][x], f)).view(np.uint32) for f in FIELDS], f"handle {k}, call {i} ({x})")
    finally:
        for m in mats:
            m.close()


@pytest.mark.parametrize("x,joined", [("A", 0), ("B", 1)], ids=["joins nothing", "joins the plan stream"])
def test_timed_span(lworld, capfd, x, joined):
    """the span of wepp_mat_last_timing -- from the end of k_route to the end of the call's last work on the caller's
    stream -- is positive and not longer than the call between two device synchronisations"""
    import torch
    mat = new_mat(lworld["g"].tree)
    try:
        lworld["dev"][x].run(mat)           # (the workspace has its size)
        if x == "A":
            lworld["dev"][x].run(mat)
        mat.timing_reset()
        torch.cuda.synchronize()
        lines(capfd)
        t0 = time.perf_counter()
        lworld["dev"][x].run(mat)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms, n_calls, _, _ = mat.last_timing()
        _, lists, info = lines(capfd)
        print(f"span {ms:.4f} ms, wall {wall_ms:.4f} ms, {lists}")
        assert info == [("report", 0, info[0][2])] and lists[0].endswith(f"joined={joined}"), (info, lists)
        assert n_calls == 1 and 0.0 < ms <= wall_ms, (ms, wall_ms)
    finally:
        mat.close()
