#!/usr/bin/env python3
"""Measurement of wepp_epp_peaks (the peak-removal loop of wepp_filter, src/WEPP/initial_filter.cpp:241-453) on the
default EPP bench shapes of tools/bench_epp.py: N-node synthetic MAT, R windowed reads.  A warm-up, then --runs calls;
prints (and with --out writes) one JSON object: wall time per call with its spread, the loop by phase
(wepp_epp_peaks_last_timing), steps, peaks and reads re-swept.

The baseline (--baseline-runs, 0 = none) drives the same loop from the host through the entry points that existed before
wepp_epp_peaks: per step wepp_epp_distances / wepp_epp_neighbors for the accepted peaks, wepp_epp_assign of the
remaining reads against them, wepp_epp_map of the removed subset (whose scores are subtracted on the host in doubles:
another scale than the resident loop's integers, so its peaks are compared, not asserted).  Its wall time includes the
host's own share (NumPy over N haplotypes and the subsets of the reads per step), as a caller composing the loop would pay."""
import argparse, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import wepp_amd as w

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--reads", type=int, default=200_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--baseline-runs", type=int, default=5)
ap.add_argument("--top-n", type=int, default=10)
ap.add_argument("--max-peaks", type=int, default=300)
ap.add_argument("--peak-radius", type=int, default=2)
ap.add_argument("--out")
a = ap.parse_args()
GENOME, EPS = 29903, 1e-9

g = w.generate_tree(21, a.nodes)
amp = max(400, a.read_len)
reads = g.reads(22, a.reads, read_len=a.read_len, amplicon_len=amp, amplicon_step=300 if a.read_len < 400 else 1000,
                windows=True, max_degree=5)
mat = w.Mat(g.tree)
N, R = g.tree.n_nodes, reads.n_reads
PAR = dict(top_n=a.top_n, max_peaks=a.max_peaks, peak_radius=a.peak_radius, score_epsilon=EPS)


def subset(idx):
    """the reads idx (ascending) as a batch of their own"""
    off = reads.read_off.astype(np.int64)
    lens = off[idx + 1] - off[idx]
    noff = np.zeros(idx.size + 1, np.uint32)
    np.cumsum(lens, out=noff[1:])
    take = np.repeat(off[idx] - noff[:-1].astype(np.int64), lens) + np.arange(int(lens.sum()), dtype=np.int64)
    return w.EppReads(noff, reads.read_word[take], reads.start[idx], reads.end[idx], reads.degree[idx])


def composed():
    """the loop through wepp_epp_map / _distances / _neighbors / _assign, its state on the host"""
    m = mat.epp_map(reads, GENOME, want_lists=False)
    score, div, P = m["score"].copy(), m["divergence"], m["max_parsimony"]
    mapped = np.zeros(N, bool)
    remaining = np.arange(R)
    peaks, steps, swept = [], 0, 0
    while len(peaks) < a.max_peaks and remaining.size:
        live = ~mapped & (score > EPS)
        if not live.any():
            break
        full = np.where(live, score * np.sqrt(div), -1.0)
        mx = full.max()
        if mx < EPS:
            break
        group = np.flatnonzero(live & (mx - full < EPS))
        acc, dist = [], []
        for c in group:
            if not (len(acc) < a.top_n and len(acc) + len(peaks) < a.max_peaks):
                break
            if all(d[c] > a.peak_radius for d in dist):
                acc.append(int(c))
                dist.append(mat.epp_distances(np.array([c], np.uint32), w.NBR_FROM_PIVOT)[0])
        sel = np.array(acc, np.uint32)
        nb = mat.epp_neighbors(sel, a.peak_radius, w.NBR_FROM_PIVOT)
        mapped[sel] = True
        mapped[nb["nbr_node"]] = True
        sub = subset(remaining)
        asg = mat.epp_assign(sub, GENOME, sel, want_lists=False)
        hit = asg["min_dist"] == P[remaining]
        if hit.any():
            gone = remaining[hit]
            score -= mat.epp_map(subset(gone), GENOME, want_counts=False, want_divergence=False, want_lists=False)["score"]
            swept += int(gone.size)
            remaining = remaining[~hit]
        peaks += acc
        steps += 1
    return dict(peaks=peaks, steps=steps, swept=swept, remaining=int(remaining.size))


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


mat.epp_peaks(subset(np.arange(64)), GENOME, want_scores=False, **PAR)            # warm-up
wall, phases, got = [], [], None
for _ in range(a.runs):
    t0 = time.perf_counter()
    got = mat.epp_peaks(reads, GENOME, want_scores=False, **PAR)
    wall.append((time.perf_counter() - t0) * 1e3)
    phases.append(w.epp_peaks_last_timing())
res = dict(kind="wepp_epp_peaks", nodes=N, reads=R, read_len=a.read_len, params=PAR,
           steps=got["n_steps"], peaks=got["n_peaks"], remaining=got["n_remaining"], reads_reswept=R - got["n_remaining"],
           wall_ms=spread(wall), phases_ms={k: spread([p[k] for p in phases]) for k in phases[0]})
if a.baseline_runs:
    bw, base = [], None
    composed()                                                                        # warm-up
    for _ in range(a.baseline_runs):
        t0 = time.perf_counter()
        base = composed()
        bw.append((time.perf_counter() - t0) * 1e3)
    same = base["peaks"] == [int(x) for x in got["peaks"]]
    res["composed"] = dict(wall_ms=spread(bw), steps=base["steps"], peaks=len(base["peaks"]), remaining=base["remaining"],
                           reads_reswept=base["swept"], same_peaks_as_resident=bool(same))
    res["resident_over_composed"] = res["wall_ms"]["median"] / res["composed"]["wall_ms"]["median"]
print(json.dumps(res))
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
