#!/usr/bin/env python3
"""Measurement of wepp_geno_diameters (the distances of dump_haplotype_uncertainty, src/WEPP/arena.cpp:494-528): one
group of 1 k, 4 k and 16 k items and 10^5 groups of 2, every item a genotype of about --entries entries at random
sites of a 29 903-site genome.  A warm-up, then --steps calls; prints (and with --out writes) one JSON object: per
configuration the device time by phase (wepp_geno_last_timing, HIP events) as medians with their spread, wall time,
pairs per second per phase, and the only baseline there is: the single-threaded merge of
wepp_amd/host/haplotype_report.cpp (mutation_distance) over the first --cpu-max-pairs pairs of the same input
(tools/diag/geno_merge_ref.cpp, built with g++ -O2; kind "port").  There is no parent-commit time: the path is new.

The CPU leg never opens the GPU: `--cpu-leg FILE` runs it alone and writes FILE, `--cpu-json FILE` reuses such a file
(it may come from another host: the file names its own)."""
import argparse, json, os, platform, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="1:1000,1:4000,1:16000,100000:2", help="groups:items per group,...")
ap.add_argument("--entries", type=int, default=100)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--cpu-max-pairs", type=int, default=2_000_000)
ap.add_argument("--out")
ap.add_argument("--cpu-leg")
ap.add_argument("--cpu-json")
a = ap.parse_args()
CONFIGS = [tuple(int(x) for x in c.split(":")) for c in a.configs.split(",")]
GENOME = 29903


def workload(groups, per):
    """items that share a pool of sites per group (as the sources of one condensed node do): 2 x entries sites, each held with probability 1/2"""
    rng = np.random.default_rng(groups * 1000003 + per)
    n = groups * per
    pool = np.sort(rng.integers(1, GENOME + 1, size=(groups, 2 * a.entries)), axis=1)
    held = rng.random((n, 2 * a.entries)) < 0.5
    pos = np.repeat(pool, per, axis=0)
    dup = np.zeros_like(held)
    dup[:, 1:] = pos[:, 1:] == pos[:, :-1]                 # (a site drawn twice is held once)
    held &= ~dup
    ref = (1 << (pos % 4)).astype(np.uint32)
    mut = rng.integers(1, 16, size=pos.shape).astype(np.uint32)
    mut = np.where(mut == ref, 15, mut).astype(np.uint32)
    words = (pos.astype(np.uint32) | (ref << 20) | (mut << 24)).astype(np.uint32)
    item_off = np.zeros(n + 1, np.uint64)
    np.cumsum(held.sum(axis=1), out=item_off[1:])
    return item_off, np.ascontiguousarray(words[held]), np.arange(0, n + 1, per, dtype=np.uint32)


def cpu_leg(path):
    out = {}
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "geno_merge_ref")
        host = os.path.join(ROOT, "wepp_amd", "host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "diag", "geno_merge_ref.cpp"),
                               os.path.join(host, "haplotype_report.cpp"), os.path.join(host, "mat.cpp"), "-o", exe, "-lz"])
        for groups, per in CONFIGS:
            item_off, words, grp_off = workload(groups, per)
            f = os.path.join(td, "in.bin")
            with open(f, "wb") as fh:
                np.array([item_off.size - 1, grp_off.size - 1], np.uint64).tofile(fh); item_off.tofile(fh); grp_off.tofile(fh); words.tofile(fh)
            out["%d:%d" % (groups, per)] = json.loads(subprocess.check_output([exe, f, str(a.cpu_max_pairs)]))
    json.dump({"host": platform.processor() or platform.machine(), "cpus": os.cpu_count(), "entries": a.entries, "configs": out}, open(path, "w"), indent=1)


if a.cpu_leg:
    cpu_leg(a.cpu_leg)
    sys.exit(0)
cpu = json.load(open(a.cpu_json)) if a.cpu_json else None

import wepp_amd as w


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


res = {"row": "geno_diameters (dump_haplotype_uncertainty's distances)", "entries": a.entries, "genome": GENOME, "configs": []}
io, wd, go = workload(1, 130)
w.geno_diameters(io, wd, go)                                # warm-up: the library's code objects, both pair forms
io, wd, go = workload(50, 2)
w.geno_diameters(io, wd, go)
for groups, per in CONFIGS:
    item_off, words, grp_off = workload(groups, per)
    pairs = groups * per * (per - 1) // 2
    walls, phases, diam = [], [], None
    for _ in range(a.steps + 1):
        t0 = time.perf_counter()
        d = w.geno_diameters(item_off, words, grp_off)
        walls.append(time.perf_counter() - t0)
        phases.append(w.geno_last_timing())
        assert diam is None or d.tobytes() == diam.tobytes()
        diam = d
    walls, phases = walls[1:], phases[1:]                   # (the first call of a size allocates)
    med = {k: statistics.median(p[k] for p in phases) for k in ("columns_ms", "planes_ms", "pairs_ms")}
    row = {"groups": groups, "items_per_group": per, "words": int(item_off[-1]), "pairs": pairs,
           "columns_ms": spread([p["columns_ms"] for p in phases]), "planes_ms": spread([p["planes_ms"] for p in phases]),
           "pairs_ms": spread([p["pairs_ms"] for p in phases]), "wall_s": spread(walls),
           "pairs_per_s": {"pairs_phase": pairs / (med["pairs_ms"] * 1e-3) if med["pairs_ms"] else None,
                           "all_phases": pairs / (sum(med.values()) * 1e-3), "wall": pairs / statistics.median(walls)},
           "diam": {"min": int(diam.min()), "max": int(diam.max())}}
    if cpu and "%d:%d" % (groups, per) in cpu["configs"]:
        c = cpu["configs"]["%d:%d" % (groups, per)]
        row["cpu_baseline"] = {"kind": "port", "host": cpu["host"], "pairs": c["pairs"], "seconds": c["seconds"], "pairs_per_s": c["pairs_per_s"],
                               "sample": "mutation_distance of haplotype_report.cpp, one thread, the first %d pairs" % c["pairs"]}
    res["configs"].append(row)
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
