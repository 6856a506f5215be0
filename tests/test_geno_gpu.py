"""wepp_geno_diameters / wepp_geno_nearest on the GPU against the literal model (tests/geno_model.py): diam, min_dist,
nearest and matrix equal, for every case of tests/geno_cases.py (each held to its edge by tests/test_geno_cases.py)
and a fuzz over the genotypes of random trees; with the case's own WEPP_GENO_PASS_BYTES, without the variable and
with one group per pass; twice on the same input for the same bytes; and the timing call."""
import math

import numpy as np
import pytest

import geno_cases as gc
import wepp_amd as w

pytestmark = pytest.mark.gpu

CASES = gc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_equals_model(case):
    gc.check(case, gc.run(case, w.geno_diameters, w.geno_nearest))
    # the pass variable changes no result: without it, and with one group per pass
    gc.check(case, gc.run(case, w.geno_diameters, w.geno_nearest, force_pass_bytes=None))
    gc.check(case, gc.run(case, w.geno_diameters, w.geno_nearest, force_pass_bytes=1))


def test_fuzz_equals_model():
    for case in gc.fuzz(20261020, 40):
        gc.check(case, gc.run(case, w.geno_diameters, w.geno_nearest))
        gc.check(case, gc.run(case, w.geno_diameters, w.geno_nearest, force_pass_bytes=None))


@pytest.mark.parametrize("name", ["sizes", "mix", "near_65x129", "near_ties"])
def test_two_calls_same_bytes(name):
    case = next(c for c in CASES if c["name"] == name)
    a = gc.run(case, w.geno_diameters, w.geno_nearest)
    b = gc.run(case, w.geno_diameters, w.geno_nearest)
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert x.tobytes() == y.tobytes()


def test_timing_is_finite():
    for name in ("mix", "near_65x129"):
        gc.run(next(c for c in CASES if c["name"] == name), w.geno_diameters, w.geno_nearest)
        t = w.geno_last_timing()
        assert set(t) == {"columns_ms", "planes_ms", "pairs_ms"}
        assert all(math.isfinite(v) and v >= 0 for v in t.values()), t
        assert t["pairs_ms"] > 0, t


def test_errors_reach_python():
    off, words = np.zeros(2, np.uint64), np.zeros(0, np.uint32)
    with pytest.raises(w.WeppError) as e:
        w.geno_diameters(off, words, np.array([0, 2], np.uint32))
    assert e.value.code == 1 and "grp_off ends at 2" in str(e.value)
