"""ctypes binding of wepp_sam_build and wepp_sam_build_subsampled (include/wepp_place.h): aligned reads -> frequency
table, order, groups and the merged batch, over all reads or over a drawn subset.  Computes nothing itself."""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, check
from .api import EppReads, _ptr

SAM_CODES = "ACGTN_"  # base byte -> character (sam2pb.hpp:10)


def _build(call, reference, start, base_off, base, min_af, min_depth, want_freq, word_capacity, so):
    """the arguments and outputs the two calls share; call(ref pointer, G, rd, par, out) -> the return code"""
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
    rc = call(_ptr(ref) if G else None, G, ctypes.byref(rd), ctypes.byref(par), ctypes.byref(o))
    M = int(n_merged[0])
    if rc == 4 and M and int(read_off[M]) > cap:
        # everything else is complete; the words wait in this thread
        words = np.zeros(int(read_off[M]), np.uint32)
        rc = so.wepp_sam_fetch_words(_ptr(words), int(read_off[M]))
    if rc:
        raise _lib.WeppError(rc, so.wepp_last_error().decode("utf-8", "replace"))
    n_words = int(read_off[M]) if M else 0
    reads = EppReads(read_off[: M + 1].copy(), words[:n_words].copy(), st[:M].copy(), en[:M].copy(), deg[:M].copy())
    return dict(freq=freq, order=order[:R], n_merged=M, group_off=group_off[: M + 1], reads=reads)


def sam_build(reference, start, base_off, base, min_af, min_depth, device=0, want_freq=True, word_capacity=None, so=lib):
    """wepp_sam_build.  reference: the reference's characters (str or bytes); start[R] 0-based, base_off[R + 1],
    base[] bytes 0..5.  Returns a dict: freq (genome x 6, or None), order, n_merged, group_off, reads (the merged
    batch as EppReads).  A short word_capacity goes through wepp_sam_fetch_words.  so: another build of the library."""
    return _build(lambda ref, G, rd, par, o: so.wepp_sam_build(int(device), ref, G, rd, par, o),
                  reference, start, base_off, base, min_af, min_depth, want_freq, word_capacity, so)


def sam_build_subsampled(reference, start, base_off, base, min_af, min_depth, seed, max_reads, trials=1000, device=0, want_freq=True,
                         word_capacity=None, so=lib):
    """wepp_sam_build_subsampled: of more than max_reads reads the best of `trials` seeded subsets is kept.  Returns
    sam_build's dict (freq = the full table; order names input reads and holds n_kept entries) plus n_kept, kept,
    best_trial (None when nothing was drawn), divergence[trials], threshold[trials].  so: another build of the library."""
    n_kept, best = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    kept = np.zeros(max(int(max_reads), 1), np.uint32)
    div, thr = np.zeros(max(int(trials), 1), np.float64), np.zeros(max(int(trials), 1), np.uint64)
    sub = _lib.SamSubsampleParamsC(int(seed), int(max_reads), int(trials))
    sub_out = _lib.SamSubsampleOutC(_ptr(n_kept).value, _ptr(kept).value, _ptr(best).value, _ptr(div).value, _ptr(thr).value)
    got = _build(lambda ref, G, rd, par, o: so.wepp_sam_build_subsampled(int(device), ref, G, rd, par, ctypes.byref(sub), o, ctypes.byref(sub_out)),
                 reference, start, base_off, base, min_af, min_depth, want_freq, word_capacity, so)
    k = int(n_kept[0])
    got.update(n_kept=k, kept=kept[:k], best_trial=None if int(best[0]) == 0xFFFFFFFF else int(best[0]), divergence=div[: int(trials)],
               threshold=thr[: int(trials)], order=got["order"][:k])
    return got


def sam_last_timing():
    """device ms of the calling thread's last wepp_sam_build: pile-up, correction, sort, merge"""
    v = [ctypes.c_double() for _ in range(4)]
    check(lib.wepp_sam_last_timing(*[ctypes.byref(x) for x in v]))
    return dict(zip(("pileup_ms", "correct_ms", "sort_ms", "merge_ms"), (x.value for x in v)))


def sam_subsample_last_timing():
    """device ms of the calling thread's last wepp_sam_build_subsampled: thresholds, trials, pick"""
    v = [ctypes.c_double() for _ in range(3)]
    check(lib.wepp_sam_subsample_last_timing(*[ctypes.byref(x) for x in v]))
    return dict(zip(("select_ms", "trials_ms", "pick_ms"), (x.value for x in v)))
