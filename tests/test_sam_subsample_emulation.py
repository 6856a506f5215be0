"""sam_subsample_capi.cpp, sam_capi.cpp and the kernels of sam_subsample_kernels.hip and sam_kernels.hip under the CPU
emulation (tests/sam_emu.py), unchanged, on the cases of tests/subsample_cases.py that are small enough for one host
thread per lane, against the model: the same demands as tests/test_sam_subsample_gpu.py makes of the device.  The
emulation shows the logic, the indexing and the buffer sizes; what only the device can show stays with the gpu tests."""
import pytest

import sam_emu
import sam_model as sm
import subsample_cases as sc
from test_sam_gpu import encode
from test_sam_subsample_gpu import check, same

SMALL = ["m1", "m257", "T7", "T9", "T17", "G256", "G517", "n512", "n513", "floors", "ties", "full_table"]


def run(name, **kw):
    ref, reads, min_af, min_depth, seed, m, T = sc.CASES[name]
    return sam_emu.sam_build_subsampled(ref, *encode(reads), min_af=min_af, min_depth=min_depth, seed=seed, max_reads=m, trials=T, **kw)


@pytest.mark.parametrize("name", SMALL)
def test_case(name):
    check(run(name), sc.model(name), name)


def test_three_passes_equal_one(monkeypatch):
    one = run("passes")
    check(one, sc.model("passes"), "passes")
    monkeypatch.setenv("WEPP_SAM_SUBSAMPLE_PASS_BYTES", str(8 * len(sc.CASES["passes"][0]) * 24))
    same(run("passes"), one)


def test_plain_build_is_unchanged_and_no_draw_equals_it():
    """the stages wepp_sam_build shares with the subsampled call, and n <= max_reads"""
    ref, reads = sm.gen_aligned(12, G=200, n_reads=130)
    m = sm.build(ref, reads, sc.AF, 3)
    want = sam_emu.sam_build(ref, *encode(reads), min_af=sc.AF, min_depth=3)
    assert want["order"].tolist() == m["order"] and want["group_off"].tolist() == m["group_off"]
    assert want["reads"].read_word.tolist() == m["read_word"] and want["reads"].degree.tolist() == m["degree"]
    got = sam_emu.sam_build_subsampled(ref, *encode(reads), min_af=sc.AF, min_depth=3, seed=1, max_reads=130, trials=5)
    assert got["best_trial"] is None and got["kept"].tolist() == list(range(130)) and not got["divergence"].any()
    for k in ("freq", "order", "group_off"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["reads"].read_word.tobytes() == want["reads"].read_word.tobytes()
