"""wepp_sam_build's argument checks, which are made before the device is touched: they run without a GPU.  (The check
of the base bytes runs on the device: tests/test_sam_gpu.py.)"""
import ctypes

import numpy as np
import pytest

import wepp_amd as w
from wepp_amd import _lib

REF = "ACGT" * 20
AF = float(np.float32("0.005"))


def test_no_reads_is_ok_and_needs_no_device():
    got = w.sam_build(REF, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint8), AF, 10)
    assert got["n_merged"] == 0 and got["group_off"].tolist() == [0] and got["reads"].n_reads == 0
    assert got["freq"].shape == (80, 6) and not got["freq"].any()


@pytest.mark.parametrize("name,want", [("start", "does not lie inside"), ("end", "does not lie inside"), ("empty", "is empty"),
                                        ("descending", "does not ascend"), ("first_offset", "base_off[0]")])
def test_invalid_windows_and_offsets(name, want):
    start, off, base = np.array([0, 70], np.uint32), np.array([0, 5, 12], np.uint64), np.zeros(12, np.uint8)
    if name == "start":
        start[1] = 80
    elif name == "end":
        start[1] = 74
    elif name == "empty":
        off[1] = 0
    elif name == "descending":
        off[1] = 13
    else:
        off[0] = 1
    with pytest.raises(w.WeppError) as ei:
        w.sam_build(REF, start, off, base, AF, 10)
    assert ei.value.code == 1 and want in str(ei.value)


def test_null_arguments_and_limits():
    assert _lib.lib.wepp_sam_build(0, None, 0, None, None, None) == 1
    with pytest.raises(w.WeppError) as ei:
        w.sam_build("A" * (0xFFFFE + 1), np.zeros(1, np.uint32), np.array([0, 1], np.uint64), np.zeros(1, np.uint8), AF, 10, want_freq=False)
    assert ei.value.code == 4 and "20-bit" in str(ei.value)
    assert _lib.lib.wepp_sam_fetch_words(None, 0) == 1 and b"pending" in _lib.lib.wepp_last_error()
    v = [ctypes.c_double(-1) for _ in range(4)]
    assert _lib.lib.wepp_sam_last_timing(*[ctypes.byref(x) for x in v]) == 0
