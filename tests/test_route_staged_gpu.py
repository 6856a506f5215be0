"""k_route's staged loads (route_kernels.hip): the first W words of a read and the routing words of their positions are
requested per phase for the four reads of a thread and kept in registers, and entries from the W-th on are loaded where
they are used.

The tree is the one of tests/test_route_tables_gpu.py (30 000 nodes over 10 000 positions, window crowns and several
tree-wide streams).  Reads are built by construction around the seam between the staged entries and the others; what
k_route makes of each is counted on the CPU (Router of that module) and compared with the kernel's own counters
(WEPP_DEBUG_PLANS=1).  Results go into device arrays filled with 0x7FFFFFFF and are compared with the incremental
checker."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import read_kinds as rk
import test_route_tables_gpu as T
import wepp_amd as w
from test_fused_step import NTHREADS, assert_checker, assert_equal, entry, position_table
from wepp_amd import Reads

HERE = os.path.dirname(os.path.abspath(__file__))
W = 4                                            # device_mat.hpp: ROUTE_STAGED_WORDS
ENTRY_COUNTS = tuple(range(10)) + (16, 17)
WAVE = 64
BLOCKS = T.ROUTE_BLOCKS


def staged_words():
    path = os.path.join(os.path.dirname(os.path.abspath(w.__file__)), "csrc", "device_mat.hpp")
    with open(path) as fh:
        return int(re.search(r"constexpr uint32_t ROUTE_STAGED_WORDS = (\d+);", fh.read()).group(1))


def kinds(tree, model, seed):
    """name -> list of samples, by construction from the tree's position table"""
    counts, ref = position_table(tree)
    counts = np.concatenate([counts, np.zeros(max(0, model.max_pos + 2 - counts.size), counts.dtype)])
    ref = np.concatenate([ref, np.zeros(counts.size - ref.size, ref.dtype)])
    ref = np.where(ref == 0, 1 << (np.arange(ref.size) % 4), ref)
    rng = np.random.default_rng(seed)
    allp = np.arange(1, model.max_pos)
    hot, cold = allp[(counts[allp] >= 1) & (counts[allp] <= 3)], allp[counts[allp] == 0]
    stride, size = model.stride, model.size
    n_win = (model.max_pos - size) // stride + 1
    out = {}

    def sample(pos):
        pos = np.sort(np.asarray(pos))
        assert np.unique(pos).size == pos.size
        return [entry(rng, p, ref) for p in pos]

    def in_window(k, n_hot):
        wi = int(rng.integers(0, n_win))
        lo, hi = wi * stride, wi * stride + size
        h, c = hot[(hot >= lo) & (hot < hi)], cold[(cold >= lo) & (cold < hi)]
        return sample(np.concatenate([rng.choice(h, n_hot, replace=False), rng.choice(c, k - n_hot, replace=False)]))

    # exactly k entries inside one window; the last word of k = W is staged, of k = W + 1 it is not
    for k in ENTRY_COUNTS:
        out[f"k{k}"] = [in_window(k, int(rng.integers(1 if k >= 9 else 0, min(k, 3) + 1))) if k else [] for _ in range(60)]
    # the only events at entry e (counted from 0): the last staged entry, the first and the second of the others
    for e in (W - 1, W, W + 1):
        seam = []
        while len(seam) < 300:
            k = int(rng.integers(e + 1, 9))
            wi = int(rng.integers(0, n_win))
            lo, hi = wi * stride, wi * stride + size
            h = int(rng.choice(hot[(hot >= lo) & (hot < hi)]))
            below, above = cold[(cold >= lo) & (cold < h)], cold[(cold > h) & (cold < hi)]
            if below.size >= e and above.size >= k - 1 - e:
                S = sample(np.concatenate([rng.choice(below, e, replace=False), [h], rng.choice(above, k - 1 - e, replace=False)]))
                assert S[e][0] == h
                seam.append(S)
        out[f"seam{e}"] = seam
    # the last head slots of a slice: an entry AT max_pos and one beyond it, as entry 1 (staged) and as entry W + 1
    tail = allp[(allp > model.max_pos - size) & (counts[allp] <= 3)]
    for name, last in (("at_max", model.max_pos), ("beyond", model.max_pos + 1)):
        for k in (2, W + 2):
            out[f"{name}_k{k}"] = [sample(np.concatenate([rng.choice(tail, k - 1, replace=False), [last]])) for _ in range(60)]
    # two windows: the first entry in window wi, the last one behind its end -- the last word staged (k = W) and not
    for k in (W, W + 1):
        span = []
        while len(span) < 100:
            a = int(rng.choice(hot[hot < model.max_pos - size - 1]))
            b = int(rng.choice(hot[hot >= (a // stride) * stride + size]))
            mid = allp[(allp > a) & (allp < b) & (counts[allp] <= 1)]
            if mid.size >= k - 2:
                span.append(sample(np.concatenate([[a, b], rng.choice(mid, k - 2, replace=False)])))
        out[f"span_k{k}"] = span
    return out


@pytest.fixture(scope="module")
def world(oracle):
    g = T.make_tree()
    fv = w.FlatView(g.tree)
    model = T.Router(fv)
    by_kind = kinds(g.tree, model, 23)
    names = np.array([n for n, v in by_kind.items() for _ in v])
    samples = [S for v in by_kind.values() for S in v]
    # mixed, so that the reads of a wave differ in their number of entries; reads without entries are the batch's last
    order = np.random.default_rng(24).permutation(len(samples))
    names, samples = np.concatenate([names[order], np.array(["tail0"] * 70)]), [samples[i] for i in order] + [[] for _ in range(70)]
    routed = [model.route(S) for S in samples]
    reads = Reads.from_lists(samples)
    many = T.many_event_reads(g.tree, model, 12, 1500)
    inc = oracle.OracleTree(g.tree).incremental()
    yield dict(g=g, fv=fv, model=model, names=names, samples=samples, routed=routed, reads=reads, inc=inc,
               want=inc.place_batch(reads, nthreads=NTHREADS), many=many, want_many=inc.place_batch(many, nthreads=NTHREADS))
    fv.close()
    g.close()


def check_batch(world):
    model, names, samples, routed = world["model"], world["names"], world["samples"], world["routed"]
    assert staged_words() == W
    assert world["fv"].n_streams >= 3 and (model.wc_n[:(model.max_pos - model.size) // model.stride + 1, 0] > 0).all()
    ks = np.array([len(S) for S in samples])
    for k in ENTRY_COUNTS:
        assert (ks[names == f"k{k}"] == k).all() and (names == f"k{k}").sum() == 60
    assert (ks[-70:] == 0).all()
    cls = np.array([c for c, _ in routed])
    assert set(cls[names == "k17"]) == {"other"} and set(cls[names == "k0"]) == {"resolved"}
    for c in ("resolved", "walk8", "walk16"):
        assert (cls == c).sum() >= 40, (c, T.model_counts(cls))
    for e in (W - 1, W, W + 1):
        seam = [(S, r) for S, n, r in zip(samples, names, routed) if n == f"seam{e}"]
        # no events at any entry but e in any table k_route consults, and events there for some
        assert all(sum(model.lens(S[:e] + S[e + 1:], st)) == 0 for S, _ in seam for st in model.streams_of(S))
        assert sum(1 for _, (c, ev) in seam if ev > 0) >= 20, e
    for k in (2, W + 2):
        assert all(len(S) == k and S[-1][0] == model.max_pos for S, n in zip(samples, names) if n == f"at_max_k{k}")
        assert all(len(S) == k and S[-1][0] == model.max_pos + 1 for S, n in zip(samples, names) if n == f"beyond_k{k}")
    for k in (W, W + 1):
        assert all(len(S) == k and S[-1][0] >= (S[0][0] // model.stride) * model.stride + model.size
                   for S, n in zip(samples, names) if n == f"span_k{k}")
        inside = [S for S, n in zip(samples, names) if n == f"k{k}"]
        assert all(S[-1][0] < (S[0][0] // model.stride) * model.stride + model.size for S in inside)
        assert sum(1 for S in inside if len(model.streams_of(S)) == 2) >= 30          # a window crown serves them


def test_batch_holds_every_kind(world):
    """On the CPU: the mixed batch holds the kinds the GPU tests are about."""
    check_batch(world)


@pytest.mark.gpu
def test_mixed_batch(world, monkeypatch, capfd):
    """Every kind against the checker, k_route's counts against the model's, and a second call on the handle."""
    check_batch(world)
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    mat = w.Mat(world["g"].tree)
    try:
        res = T.place_filled(mat, world["reads"])
        c = T.route_counts(capfd)
        assert_checker(res, world["want"], "mixed batch")
        want = T.model_counts([x for x, _ in world["routed"]])
        assert {k: c[k] for k in want} == want and c["reads"] == world["reads"].n_reads, (c, want)
        assert_equal(T.place_filled(mat, world["reads"]), res, "second call")
    finally:
        mat.close()


def wave_batch(world, with_one_above):
    """64 reads a routing block -- one wave, one read a lane.  with_one_above: every lane has at most two entries but
    one, which has W + 1; else no lane has more than W (the wave issues no load outside the staged sets)."""
    ks = np.array([len(S) for S in world["samples"]])
    ok = np.array([c != "other" for c, _ in world["routed"]])
    low = np.flatnonzero(ok & (ks <= 2)) if with_one_above else np.flatnonzero(ok & (ks <= W))
    five = np.flatnonzero(ok & (ks == W + 1))
    assert low.size >= 200 and five.size >= 100
    idx = np.resize(low, BLOCKS * WAVE).reshape(BLOCKS, WAVE)
    if with_one_above:
        for b in range(BLOCKS):
            idx[b, (b * 7) % WAVE] = five[b % five.size]
    assert ((ks[idx] > W).sum(1) == (1 if with_one_above else 0)).all()
    return idx.reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("with_one_above", [True, False], ids=["one lane beyond the staged words", "no lane beyond"])
def test_waves_by_their_longest_read(world, monkeypatch, capfd, with_one_above):
    """Results and k_route's counts for waves whose lanes run the generic loops for one lane only, or for none.  What
    such a wave saves -- it branches over every load for entries from the W-th on -- changes no result and cannot fail
    here: it is read from the machine code (profiles/r24_route_loads/loads_and_waits.txt)."""
    idx = wave_batch(world, with_one_above)
    assert -(-idx.size // BLOCKS) == WAVE
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    mat = w.Mat(world["g"].tree)
    try:
        res = T.place_filled(mat, rk.take(world["reads"], idx))
        c = T.route_counts(capfd)
        assert_checker(res, world["want"][idx], "waves")
        want = T.model_counts([world["routed"][i][0] for i in idx])
        assert {k: c[k] for k in want} == want and c["reads"] == idx.size, (c, want)
    finally:
        mat.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_batch_sizes(world, n):
    """Fewer reads than routing blocks, a block without a read, two reads in a block, and a thread's second read."""
    idx = np.resize(np.arange(world["reads"].n_reads - 70), n) if n > 1 else np.flatnonzero(world["names"] == f"k{W + 1}")[:1]
    mat = w.Mat(world["g"].tree)
    try:
        assert_checker(T.place_filled(mat, rk.take(world["reads"], idx)), world["want"][idx], f"{n} reads")
    finally:
        mat.close()


@pytest.mark.gpu
def test_batch_without_words(world):
    """Reads without entries only: the words' buffer is one word nobody may load; every read is placed at the root's aggregate."""
    reads = rk.empty_reads(300)
    assert reads.read_word.size == 0 and int(reads.read_off[-1]) == 0
    mat = w.Mat(world["g"].tree)
    try:
        assert_checker(T.place_filled(mat, reads), world["inc"].place_batch(reads, nthreads=NTHREADS), "no words")
    finally:
        mat.close()


@pytest.mark.gpu
def test_step_forms(world, monkeypatch):
    """The mixed batch and the reads of many events by every other form of the step: the same four arrays."""
    reads = rk.concat([world["reads"], world["many"]])
    want = np.concatenate([world["want"], world["want_many"]])
    mat = w.Mat(world["g"].tree)
    try:
        res = T.place_filled(mat, reads)
    finally:
        mat.close()
    assert_checker(res, want, "default step")
    for env in ({"WEPP_STEP_UNFUSED": "1"}, {"WEPP_STEP_GROUPS": "0"}, {"WEPP_STEP_UNFUSED": "1", "WEPP_STEP_GROUPS": "0"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m2 = w.Mat(world["g"].tree)           # (the switches are read when the handle is created)
        try:
            assert_equal(T.place_filled(m2, reads), res, str(env))
        finally:
            m2.close()


@pytest.mark.gpu
def test_second_round_of_a_block(world):
    """1 048 576 + 300 reads in one call -- 4 098 a routing block, two more than a round takes: the registers of the
    staged words are used twice -- equal the same reads placed by two calls; 512 of them
    against the checker."""
    g = world["g"]
    reads = g.reads(31, 1_048_576 + 300, read_len=150, amplicon_len=400, amplicon_step=300, p_substitution=0.001, p_n=0.005)
    assert -(-reads.n_reads // BLOCKS) > 4 * 1024
    half = reads.n_reads // 2
    mat = w.Mat(g.tree)
    try:
        res = T.place_filled(mat, reads)
        a = T.place_filled(mat, rk.take(reads, np.arange(half)))
        b = T.place_filled(mat, rk.take(reads, np.arange(half, reads.n_reads)))
    finally:
        mat.close()
    for f in ("best_bfs_j", "score", "num_best", "flags"):
        assert (getattr(res, f) == np.concatenate([getattr(a, f), getattr(b, f)])).all(), f
    idx = np.sort(np.random.default_rng(7).choice(reads.n_reads, 512, replace=False))
    assert_checker(w.PlacementResult(*[getattr(res, f)[idx] for f in ("best_bfs_j", "score", "num_best", "flags")]),
                   world["inc"].place_batch(rk.take(reads, idx), nthreads=NTHREADS), "512 sampled reads")


@pytest.fixture(scope="module")
def nested(oracle):
    g = T.make_nested_tree()
    fv = w.FlatView(g.tree)
    samples = T.refused_reads(g.tree, T.Router(fv), 13, 120)
    reads = Reads.from_lists(samples) if samples else rk.empty_reads(0)
    want = oracle.OracleTree(g.tree).incremental().place_batch(reads, nthreads=NTHREADS) if samples else None
    yield dict(g=g, samples=samples, reads=reads, want=want)
    fv.close()
    g.close()


@pytest.mark.gpu
def test_second_table_of_a_refused_read(nested):
    """Reads a window crown refuses: the second classification asks a table other than the one phase A staged words of,
    for the staged entries and the others."""
    assert len(nested["samples"]) >= 100 and all(len(S) > W for S in nested["samples"])
    mat = w.Mat(nested["g"].tree)
    try:
        assert_checker(T.place_filled(mat, nested["reads"]), nested["want"], "reads their window crown refuses")
    finally:
        mat.close()


def saturating_at(model, S, staged):
    """a list of T.SAT_LEN events or more at a staged entry (or at one of the others) in a table k_route consults"""
    idx = range(min(W, len(S))) if staged else range(W, len(S))
    return any(n >= T.SAT_LEN for st in model.streams_of(S) for j in idx for n in model.lens([S[j]], st))


@pytest.mark.gpu
def test_saturated_length_at_a_staged_position(world):
    """The rtlen3 build (length fields of 3 bits) in a child process: reads whose saturated field is a staged word, and
    reads where it is a word of the generic loop; the four arrays equal the checker's and the default build's."""
    model = world["model"]
    lists = T.to_lists(world["many"])
    staged = np.flatnonzero([saturating_at(model, S, True) for S in lists])
    late = np.flatnonzero([saturating_at(model, S, False) for S in lists])
    assert staged.size >= 300 and late.size >= 30, (staged.size, late.size)
    idx = np.unique(np.concatenate([staged[:600], late[:300]]))
    reads, want = rk.take(world["many"], idx), world["want_many"][idx]
    mat = w.Mat(world["g"].tree)
    try:
        res = T.place_filled(mat, reads)
    finally:
        mat.close()
    assert_checker(res, want, "default build")
    lib = T.variant_lib("rtlen3", "-DWEPP_RT_LEN_BITS=3")
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), read_off=reads.read_off, read_word=reads.read_word)
        run = subprocess.run([sys.executable, os.path.join(HERE, "route_variant_child.py"), os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")],
                             env=dict(os.environ, WEPP_PLACE_LIB=lib), capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
        assert json.loads(run.stdout.strip().splitlines()[-1])["len_bits"] == 3
        out = np.load(os.path.join(tmp, "out.npz"))
        got = w.PlacementResult(out["best_bfs_j"], out["score"], out["num_best"], out["flags"])
    assert_checker(got, want, "length fields of 3 bits")
    assert_equal(got, res, "length fields of 3 bits against the default build")
