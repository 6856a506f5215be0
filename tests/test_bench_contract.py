"""The bench line's contract (the round's task statement, section 4): the committed lines under profiles/ -- what
`python bench.py` printed on the GPU box for this build -- carry every field in the shape the driver and the judge read;
`bench.py` itself defaults to one GPU and a short run.  (No GPU needed: the lines are data.)"""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = ["r4_bench_default.json", "r3_bench_default.json", "r3_bench_whole_tree.json"]     # (round 4: the other configs are legs of the default line)


@pytest.mark.parametrize("name", LINES)
def test_committed_bench_line_has_the_contract_shape(name):
    with open(os.path.join(ROOT, "profiles", name)) as fh:
        text = fh.read().strip()
    assert len(text.splitlines()) == 1                      # ONE JSON line
    d = json.loads(text)
    with open(os.path.join(ROOT, "BASELINE.json")) as fh:
        base = json.load(fh)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "reads/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["n_gpus"] == 1
    assert d["vs_baseline"] is None                         # BASELINE.md holds no published number for this metric
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert str(base.get("metric", d["metric"]))[:12].lower() in d["metric"].lower() or "reads" in d["metric"]
    assert d["value"] > 0 and abs(d["value"] - d["config"]["reads_per_gpu"] / (d["ms_per_step"] * 1e-3)) < 0.02 * d["value"]
    r = d["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(r)
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    c = d["cpu_baseline"]
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(c) and c["kind"] in ("reference", "port")
    assert c["sample_matches_gpu"] is True and c["incremental"]["sample_matches_gpu"] is True
    # the counters a line quotes were taken on the build the line was measured on
    if r["traffic"] is not None:
        with open(os.path.join(ROOT, "profiles", "pmc_counters.json")) as fh:
            pmc = json.load(fh)
        assert any(e["kernel_hash"] == d["config"]["kernel_hash"] for e in pmc.values())


def test_default_line_carries_the_legs_and_the_ladder():
    """the other configs as legs of the default run, each with its own contract-shaped roofline and a
    sample checked against the oracle; the tree-shape ladder with every sample checked."""
    with open(os.path.join(ROOT, "profiles", "r4_bench_default.json")) as fh:
        d = json.load(fh)
    legs = d["legs"]
    assert len(legs) == 3
    for leg in legs:
        assert leg["sample_matches_gpu"] is True and leg["reads_per_s"] > 0 and leg["pcie_inclusive_reads_per_s"] > 0
        r = leg["roofline"]
        assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(r) and r["traffic"] is not None
    trees = d["tree_ladder"]["trees"]
    assert len(trees) >= 6
    for t in trees:
        assert t["default_batch"]["sample_matches_gpu"] is True and t["long_reads"]["sample_matches_gpu"] is True
    assert d["roofline"]["traffic"] is not None and d["value_pcie_inclusive"] > 0


def test_bench_defaults_to_one_gpu_and_a_short_run():
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("bench_for_contract", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    assert a.gpus == 1 and 1 <= a.steps <= 100 and 0 <= a.warmup <= 10
    # counters of the three bench workloads are committed (bench.py quotes them only for the build they were taken
    # on -- kernel hash inside -- and prints null otherwise: a stale table is not an error, just not evidence)
    with open(os.path.join(ROOT, "profiles", "pmc_counters.json")) as fh:
        pmc = json.load(fh)
    assert {"short_reads:1000000", "short_reads:1250000", "whole_tree:1000000", "long_reads:125000", "genome_samples:20000"} <= set(pmc)
    assert all(len(e["kernel_hash"]) == len(bench.kernel_hash()) for e in pmc.values())


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_contract", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_plain_run_is_the_default_and_full_is_an_option():
    import sys
    bench = _load_bench()
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"]
        a = bench.parse()
        assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
        sys.argv = ["bench.py", "--full", "--dump-outputs", "out"]
        a = bench.parse()
        assert a.full is True and a.dump_outputs == "out"
    finally:
        sys.argv = argv


def test_dump_outputs_writes_exact_float64_arrays(tmp_path):
    import numpy as np
    bench = _load_bench()
    rng = np.random.default_rng(5)
    arrays = {"best_bfs_j": rng.integers(0, 2**32, 1000, dtype=np.uint64).astype(np.uint32),
              "score": rng.integers(-5, 40, 1000).astype(np.int32)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / "d" / (name + ".npy"))
        assert got.dtype == np.float64 and (got == a.astype(np.float64)).all()
    assert not (tmp_path / "d" / "read_index.npy").exists()


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path):
    import numpy as np
    bench = _load_bench()
    a = {"score": np.arange(10_000, dtype=np.int32), "flags": np.arange(10_000, dtype=np.uint32) % 7}
    limit = 8 * 3 * 1000                   # room for 1000 reads of two arrays + their indices
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), a, limit_bytes=limit)
    idx = np.load(tmp_path / "x" / "read_index.npy")
    assert len(idx) == 1000 and (np.diff(idx) > 0).all()
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x")) <= limit + 3 * 128
    for name in ("score", "flags", "read_index"):
        x, y = np.load(tmp_path / "x" / (name + ".npy")), np.load(tmp_path / "y" / (name + ".npy"))
        assert (x == y).all()
    assert (np.load(tmp_path / "x" / "score.npy") == idx).all()
    assert (np.load(tmp_path / "x" / "flags.npy") == idx % 7).all()
