"""ctypes binding of wepp_sam_build (include/wepp_place.h): aligned reads -> frequency table, order, groups and the
merged batch.  Computes nothing itself."""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, check
from .api import EppReads, _ptr

SAM_CODES = "ACGTN_"  # base byte -> character (sam2pb.hpp:10)


def sam_build(reference, start, base_off, base, min_af, min_depth, device=0, want_freq=True, word_capacity=None):
    """wepp_sam_build.  reference: the reference's characters (str or bytes); start[R] 0-based, base_off[R + 1],
    base[] bytes 0..5.  Returns a dict: freq (genome x 6, or None), order, n_merged, group_off, reads (the merged
    batch as EppReads).  A short word_capacity goes through wepp_sam_fetch_words."""
    ref = np.frombuffer(reference.encode() if isinstance(reference, str) else bytes(reference), np.uint8)
    G = int(ref.size)
    start = np.ascontiguousarray(start, np.uint32)
    base_off = np.ascontiguousarray(base_off, np.uint64)
    base = np.ascontiguousarray(base, np.uint8)
    R = int(start.size)
    freq = np.zeros((G, 6), np.int32) if want_freq else None
    n_merged = np.zeros(1, np.uint32)
    order = np.zeros(max(R, 1), np.uint32)
    group_off = np.zeros(R + 1, np.uint32)
    read_off = np.zeros(R + 1, np.uint32)
    st, en, deg = (np.zeros(max(R, 1), np.int32) for _ in range(3))
    cap = int(base.size if word_capacity is None else word_capacity)
    words = np.zeros(max(cap, 1), np.uint32)
    rd = _lib.SamReadsC(R, _ptr(start).value if R else None, _ptr(base_off).value, _ptr(base).value if base.size else None)
    par = _lib.SamParamsC(float(min_af), int(min_depth))
    o = _lib.SamOutC(_ptr(freq).value if want_freq and G else None, _ptr(n_merged).value, _ptr(order).value, _ptr(group_off).value,
                     _ptr(read_off).value, _ptr(words).value if cap else None, _ptr(st).value, _ptr(en).value, _ptr(deg).value, cap)
    rc = lib.wepp_sam_build(int(device), _ptr(ref) if G else None, G, ctypes.byref(rd), ctypes.byref(par), ctypes.byref(o))
    M = int(n_merged[0])
    if rc == 4 and M and int(read_off[M]) > cap:
        # everything else is complete; the words wait in this thread
        words = np.zeros(int(read_off[M]), np.uint32)
        check(lib.wepp_sam_fetch_words(_ptr(words), int(read_off[M])))
    else:
        check(rc)
    n_words = int(read_off[M]) if M else 0
    reads = EppReads(read_off[: M + 1].copy(), words[:n_words].copy(), st[:M].copy(), en[:M].copy(), deg[:M].copy())
    return dict(freq=freq, order=order[:R], n_merged=M, group_off=group_off[: M + 1], reads=reads)


def sam_last_timing():
    """device ms of the calling thread's last wepp_sam_build: pile-up, correction, sort, merge"""
    v = [ctypes.c_double() for _ in range(4)]
    check(lib.wepp_sam_last_timing(*[ctypes.byref(x) for x in v]))
    return dict(zip(("pileup_ms", "correct_ms", "sort_ms", "merge_ms"), (x.value for x in v)))
