"""wepp_sam_build_subsampled on the GPU against the model (tests/subsample_model.py) on the cases of
tests/subsample_cases.py: kept, n_kept, best_trial, thresholds, the full table, order, groups and the merged batch are
EQUAL; divergence[t] lies within bound_t = 4 (terms + 8) 2^-52 sum |term| of the model's exactly summed value.
tests/test_subsample_model.py shows on the CPU that in every case the winner is separated from every trial of another
table by more than the two bounds, so the equal winner is a fair demand, and that each case shows the edge it is named
after.

Layout units whose two sides are covered (wepp_amd/csrc/sam_subsample.hpp): B = 8 trials per batch (1, 7, 8, 9, 17
trials); tiles of 256 sites (255, 256, 257, 517 sites, reads that straddle, end at and start at every boundary);
chunks of 512 list entries (511, 512, 513 reads on one tile); 4096 reads per histogram workgroup (4095, 4096, 4097);
subsets of 1, n - 1 and around 64 and 256 reads; 32-bit counters beyond 65 535; passes of trials under a lowered byte
bound."""
import numpy as np
import pytest

import sam_model as sm
import subsample_cases as sc
import wepp_amd as w
from test_sam_gpu import encode

pytestmark = pytest.mark.gpu


def run(name, **kw):
    ref, reads, min_af, min_depth, seed, m, T = sc.CASES[name]
    return w.sam_build_subsampled(ref, *encode(reads), min_af=min_af, min_depth=min_depth, seed=seed, max_reads=m, trials=T, **kw)


def check(got, m, tag=""):
    T = len(m["threshold"])
    assert got["n_kept"] == len(m["kept"]) and got["kept"].tolist() == m["kept"], (tag, "kept")
    assert got["threshold"].tolist() == m["threshold"], (tag, "threshold")
    worst = max((abs(float(got["divergence"][t]) - m["divergence"][t]) / m["bound"][t] if m["bound"][t] else 0.0) for t in range(T))
    print(f"{tag}: best {got['best_trial']} (model {m['best_trial']}), largest |D - model| / bound = {worst:.3g}")
    for t in range(T):
        assert abs(float(got["divergence"][t]) - m["divergence"][t]) <= m["bound"][t], (tag, "divergence", t, got["divergence"][t], m["divergence"][t], m["bound"][t])
    assert got["best_trial"] == m["best_trial"], (tag, "best_trial")
    assert np.array_equal(got["freq"], np.array(m["freq"], np.int32).reshape(-1, 6)), (tag, "freq")
    assert got["order"].tolist() == m["order"], (tag, "order")
    assert got["n_merged"] == len(m["start"]), (tag, "n_merged")
    assert got["group_off"].tolist() == m["group_off"], (tag, "group_off")
    rd = got["reads"]
    assert rd.start.tolist() == m["start"] and rd.end.tolist() == m["end"], (tag, "windows")
    assert rd.degree.tolist() == m["degree"], (tag, "degree")
    assert rd.read_off.tolist() == m["read_off"], (tag, "read_off")
    assert rd.read_word.tolist() == m["read_word"], (tag, "read_word")


def same(a, b):
    for k in ("kept", "threshold", "divergence", "freq", "order", "group_off"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert (a["n_kept"], a["best_trial"], a["n_merged"]) == (b["n_kept"], b["best_trial"], b["n_merged"])
    for k in ("read_off", "read_word", "start", "end", "degree"):
        assert getattr(a["reads"], k).tobytes() == getattr(b["reads"], k).tobytes(), k


@pytest.mark.parametrize("name", [k for k in sorted(sc.CASES) if k not in ("ties", "passes", "full_table")])
def test_case(name):
    check(run(name), sc.model(name), name)


def test_ties_go_to_trial_0():
    """all reads are equal: every trial has the same table, so every divergence is the same double and trial 0 wins"""
    got = run("ties")
    assert len(set(got["divergence"].tolist())) == 1 and got["best_trial"] == 0
    check(got, sc.model("ties"), "ties")


def test_three_passes_equal_one(monkeypatch):
    """20 trials under a bound of 8 tables: passes of 8, 8 and 4 trials"""
    one = run("passes")
    check(one, sc.model("passes"), "passes")
    monkeypatch.setenv("WEPP_SAM_SUBSAMPLE_PASS_BYTES", str(8 * len(sc.CASES["passes"][0]) * 24))
    same(run("passes"), one)


def test_correction_follows_the_full_table():
    ref, reads, min_af, min_depth, seed, m, T = sc.CASES["full_table"]
    got, model = run("full_table"), sc.model("full_table")
    check(got, model, "full_table")
    alone = w.sam_build(ref, *encode([reads[i] for i in model["kept"]]), min_af=min_af, min_depth=min_depth)
    assert alone["reads"].read_word.tolist() != got["reads"].read_word.tolist()


@pytest.mark.parametrize("m", [130, 200])
def test_no_draw_is_sam_build(m):
    ref, reads = sm.gen_aligned(12, G=200, n_reads=130)
    got = w.sam_build_subsampled(ref, *encode(reads), min_af=sc.AF, min_depth=3, seed=1, max_reads=m, trials=5)
    want = w.sam_build(ref, *encode(reads), min_af=sc.AF, min_depth=3)
    assert got["n_kept"] == 130 and got["kept"].tolist() == list(range(130)) and got["best_trial"] is None
    assert not got["divergence"].any() and not got["threshold"].any()
    for k in ("freq", "order", "group_off"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["n_merged"] == want["n_merged"]
    for k in ("read_off", "read_word", "start", "end", "degree"):
        assert getattr(got["reads"], k).tobytes() == getattr(want["reads"], k).tobytes(), k
    assert w.sam_subsample_last_timing() == dict(select_ms=0.0, trials_ms=0.0, pick_ms=0.0)


def test_two_runs_are_bit_identical():
    same(run("G517"), run("G517"))
    t = w.sam_subsample_last_timing()
    assert t["select_ms"] > 0 and t["trials_ms"] > 0 and t["pick_ms"] > 0


def test_short_word_buffer_and_fetch():
    m = sc.model("T9")
    assert len(m["read_word"]) > 4
    for cap in (0, len(m["read_word"]) - 1):
        check(run("T9", word_capacity=cap), m, cap)


@pytest.mark.parametrize("name,code,want", [("max_reads", 1, "max_reads"), ("trials", 1, "trials"), ("many_trials", 4, "65536")])
def test_invalid(name, code, want):
    ref, reads = sm.gen_aligned(12, G=200, n_reads=130)
    m, T = {"max_reads": (0, 5), "trials": (10, 0), "many_trials": (10, 65537)}[name]
    with pytest.raises(w.WeppError) as ei:
        w.sam_build_subsampled(ref, *encode(reads), min_af=sc.AF, min_depth=3, seed=1, max_reads=m, trials=T)
    assert ei.value.code == code and want in str(ei.value)
