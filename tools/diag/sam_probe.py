#!/usr/bin/env python3
"""Measurement of wepp_sam_build (sam::build of `wepp sam2PB`, src/WEPP/sam2pb.cpp:262-314, 456-470): R aligned reads
of --read-len columns over a 29 903-site genome, amplicon starts, about 70 % duplicates.  A warm-up, then --runs calls;
prints (and with --out writes) one JSON object: the call's wall time with its spread (host buffers in, host buffers
out: the upload of the bases and the download of the results are inside) and the four device phases of
wepp_sam_last_timing.

Beside it (--host-runs, 0 = none) a single-threaded host restatement of the same steps, written for this probe in NumPy:
the table by bincount, the correction as a table lookup, the order by one sort of fixed-width byte records
(start, corrected string in ASCII order), the merge by a comparison of neighbours.  It is not the reference's code (a
std::sort of strings under TBB's scheduler, the table under one mutex) and says nothing about it; it is what a caller
without the device would run.  Its table, merged-read count and degrees are compared with the device's.
The SAM parse is host time in either case and is not part of these numbers."""
import argparse, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import wepp_amd as w

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host-runs", type=int, default=3)
ap.add_argument("--out")
a = ap.parse_args()
GENOME, L, R = 29903, a.read_len, a.reads
MIN_AF, MIN_DEPTH = float(np.float32("0.005")), 10

rng = np.random.default_rng(31)
ref_codes = rng.integers(0, 4, GENOME, dtype=np.uint8)
reference = bytes(np.frombuffer(b"ACGT", np.uint8)[ref_codes])
n_amp = (GENOME - L) // 250
amp = rng.integers(0, n_amp, R)
start = (amp * 250).astype(np.uint32)
variant = rng.integers(0, 4, R)                       # a few haplotypes per amplicon
private = rng.random(R) < 0.3                         # ... and 30 % of the reads with two errors of their own
base = np.empty((R, L), np.uint8)
CH = 1 << 20
for lo in range(0, R, CH):
    hi = min(R, lo + CH)
    b = ref_codes[start[lo:hi, None].astype(np.int64) + np.arange(L)]
    rows = np.arange(hi - lo)
    for v in range(1, 4):
        for k in range(v):
            m = variant[lo:hi] == v
            cols = (amp[lo:hi] * 7 + v * 13 + k * 31) % L
            b[rows[m], cols[m]] = (b[rows[m], cols[m]] + 1 + k) % 4
    m = private[lo:hi]
    for _ in range(2):                                # (two columns: a rare allele becomes N, and one N column alone would merge again)
        b[rows[m], rng.integers(0, L, int(m.sum()))] = rng.integers(0, 6, int(m.sum()), dtype=np.uint8)
    base[lo:hi] = b
base_off = (np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
flat = base.reshape(-1)


def host_build():
    """steps 2-4 on one host thread"""
    freq = np.zeros(GENOME * 6, np.int64)
    for lo in range(0, R, CH):
        hi = min(R, lo + CH)
        cell = (start[lo:hi, None].astype(np.int64) + np.arange(L)) * 6 + base[lo:hi]
        freq += np.bincount(cell[base[lo:hi] != 4], minlength=GENOME * 6)
    freq = freq.reshape(GENOME, 6)
    total = freq.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        is_n = (MIN_DEPTH > total)[:, None] | (MIN_AF - freq.astype(np.float64) / total[:, None].astype(np.float64) > 1e-9)
    keep = np.where(is_n, 4, np.arange(6)[None, :]).astype(np.uint8)
    keep[keep == 5] = 4
    ascii_rank = np.array([0, 1, 2, 4, 3], np.uint8)[keep]           # A < C < G < N < T
    rec = np.empty((R, 4 + L), np.uint8)
    rec[:, :4] = start.astype(">u4").view(np.uint8).reshape(R, 4)
    for lo in range(0, R, CH):
        hi = min(R, lo + CH)
        rec[lo:hi, 4:] = ascii_rank[start[lo:hi, None].astype(np.int64) + np.arange(L), base[lo:hi]]
    keys = rec.view(np.dtype((np.void, 4 + L))).reshape(R)
    order = np.argsort(keys, kind="stable")
    srt = rec[order]
    head = np.ones(R, bool)
    head[1:] = (srt[1:] != srt[:-1]).any(1)
    group_off = np.flatnonzero(head)
    degree = np.diff(np.append(group_off, R))
    return freq, order, degree


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


small = 4096
w.sam_build(reference, start[:small], base_off[:small + 1], flat[:small * L], MIN_AF, MIN_DEPTH)      # warm-up
wall, phases, got = [], [], None
for _ in range(a.runs):
    t0 = time.perf_counter()
    got = w.sam_build(reference, start, base_off, flat, MIN_AF, MIN_DEPTH)
    wall.append((time.perf_counter() - t0) * 1e3)
    phases.append(w.sam_last_timing())
res = dict(kind="wepp_sam_build", reads=R, read_len=L, genome=GENOME, merged=got["n_merged"], duplicate_share=1 - got["n_merged"] / R,
           words=int(got["reads"].read_word.size), wall_ms=spread(wall), phases_ms={k: spread([p[k] for p in phases]) for k in phases[0]})
if a.host_runs:
    hw, host = [], None
    for _ in range(a.host_runs):
        t0 = time.perf_counter()
        host = host_build()
        hw.append((time.perf_counter() - t0) * 1e3)
    same = (np.array_equal(host[0], got["freq"]) and host[2].size == got["n_merged"] and np.array_equal(host[2], got["reads"].degree)
            and np.array_equal(host[1].astype(np.uint32), got["order"]))
    res["host"] = dict(wall_ms=spread(hw), same_table_order_and_degrees=bool(same))
    res["device_over_host"] = res["wall_ms"]["median"] / res["host"]["wall_ms"]["median"]
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
