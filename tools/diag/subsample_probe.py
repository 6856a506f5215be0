#!/usr/bin/env python3
"""Measurement of wepp_sam_build_subsampled (sam::subsample in front of sam::build, src/WEPP/sam2pb.cpp:362-454) on the
input of tools/diag/sam_probe.py: R aligned reads of --read-len columns over a 29 903-site genome, amplicon starts.  For
every --max-reads M: a warm-up, then --runs calls with --trials trials; the call's wall time (host buffers in, host
buffers out) and the three device phases of wepp_sam_subsample_last_timing, medians with their spread.

The yardstick is what a loop over the trials with the one-table pile-up would cost: trials x pileup_ms of wepp_sam_build
on the M kept reads (k_sam_pileup with the keep table, wepp_sam_last_timing), measured in the same process.  It leaves
out what such a loop would also need per trial (the draw, the compaction of the subset, the divergence), so it flatters
the loop.  Prints (and with --out writes) one JSON object."""
import argparse, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import wepp_amd as w

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--max-reads", type=int, nargs="+", default=[1_000_000, 5_000_000])
ap.add_argument("--trials", type=int, default=1000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out")
a = ap.parse_args()
GENOME, L, R = 29903, a.read_len, a.reads
MIN_AF, MIN_DEPTH = float(np.float32("0.005")), 10

# the reads of sam_probe.py, drawn the same way
rng = np.random.default_rng(31)
ref_codes = rng.integers(0, 4, GENOME, dtype=np.uint8)
reference = bytes(np.frombuffer(b"ACGT", np.uint8)[ref_codes])
n_amp = (GENOME - L) // 250
amp = rng.integers(0, n_amp, R)
start = (amp * 250).astype(np.uint32)
variant = rng.integers(0, 4, R)
private = rng.random(R) < 0.3
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
    for _ in range(2):
        b[rows[m], rng.integers(0, L, int(m.sum()))] = rng.integers(0, 6, int(m.sum()), dtype=np.uint8)
    base[lo:hi] = b
base_off = (np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
flat = base.reshape(-1)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


small = 4096
w.sam_build_subsampled(reference, start[:small], base_off[:small + 1], flat[:small * L], MIN_AF, MIN_DEPTH, a.seed, small // 2, 16, want_freq=False)   # warm-up
res = dict(kind="wepp_sam_build_subsampled", reads=R, read_len=L, genome=GENOME, trials=a.trials, seed=a.seed, cases=[])
for M in a.max_reads:
    wall, phases, build, got = [], [], [], None
    for _ in range(a.runs + 1):                                         # (the first call at this size is a warm-up too)
        t0 = time.perf_counter()
        got = w.sam_build_subsampled(reference, start, base_off, flat, MIN_AF, MIN_DEPTH, a.seed, M, a.trials, want_freq=False)
        wall.append((time.perf_counter() - t0) * 1e3)
        phases.append(w.sam_subsample_last_timing())
        build.append(w.sam_last_timing())
    wall, phases, build = wall[1:], phases[1:], build[1:]
    # the yardstick: the one-table pile-up over the M kept reads
    kept = got["kept"].astype(np.int64)
    k_start, k_flat = start[kept], base[kept].reshape(-1)
    k_off = (np.arange(M + 1, dtype=np.uint64) * np.uint64(L))
    pile = []
    for _ in range(a.runs + 1):
        w.sam_build(reference, k_start, k_off, k_flat, MIN_AF, MIN_DEPTH, want_freq=False)
        pile.append(w.sam_last_timing()["pileup_ms"])
    pile = pile[1:]
    case = dict(max_reads=M, best_trial=got["best_trial"], divergence=float(got["divergence"][got["best_trial"]]), merged=got["n_merged"],
                wall_ms=spread(wall), phases_ms={k: spread([p[k] for p in phases]) for k in phases[0]},
                sam_phases_ms={k: spread([p[k] for p in build]) for k in build[0]},
                one_table_pileup_ms=spread(pile), loop_of_pileups_ms=a.trials * statistics.median(pile))
    case["trials_over_loop"] = case["phases_ms"]["trials_ms"]["median"] / case["loop_of_pileups_ms"]
    res["cases"].append(case)
    print(json.dumps(case), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
