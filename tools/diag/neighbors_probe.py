#!/usr/bin/env python3
"""Measurement of wepp_epp_neighbors (arena::closest_neighbors / highest_scoring_neighbors, src/WEPP/arena.cpp:171-249):
N-node synthetic MAT (--p-hub: the generator's share of hub children), per configuration K pivots drawn with a seed
and a radius.  A warm-up, then --steps calls that ask for the sizes only and -- when the lists stay under
--max-list-entries -- one call that fetches them; prints (and with --out writes) one JSON object: the device time by
phase (wepp_epp_neighbors_last_timing, HIP events, summed over the passes) with its spread, wall time, the list
sizes, and the only baseline there is: the host time of the reference's local BFS (closest_neighbors restated in
Python, list merges over stack_muts built on demand; tests/neighbors_model.py is the same code over a whole arena)
for --cpu-pivots of the pivots, each stopped after --cpu-max-visits probes (kind: "port").

The CPU leg never opens the GPU: `--cpu-leg FILE` runs it alone and writes FILE, `--cpu-json FILE` reuses such a file
(it may come from another host: the file names its own), otherwise it runs first in a child process."""
import argparse, json, os, platform, statistics, subprocess, sys, tempfile, time
from collections import deque
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wepp_amd as w

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--p-hub", type=float, default=None)
ap.add_argument("--configs", default="300:2,5000:6", help="K:radius,...")
ap.add_argument("--form", type=int, default=w.NBR_TO_PIVOT)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--max-list-entries", type=int, default=100_000_000)
ap.add_argument("--cpu-pivots", type=int, default=20)
ap.add_argument("--cpu-max-visits", type=int, default=20000)
ap.add_argument("--out")
ap.add_argument("--cpu-leg")
ap.add_argument("--cpu-json")
a = ap.parse_args()
CONFIGS = [tuple(int(x) for x in c.split(":")) for c in a.configs.split(",")]


def workload():
    kw = {} if a.p_hub is None else {"p_hub": a.p_hub}
    g = w.generate_tree(21, a.nodes, **kw)
    pivots = {K: np.random.default_rng(23 + K).permutation(g.tree.n_nodes)[:K].astype(np.uint32) for K, _ in CONFIGS}
    return g, pivots


# ---- the CPU leg ---------------------------------------------------------------------------------------------
def cpu_leg(path):
    from neighbors_model import mutation_distance
    g, pivots = workload()
    fv = w.FlatView(g.tree)
    woff, words, par = fv.get("node_woff").copy(), fv.get("words").copy(), fv.get("parent_dfs").copy()
    fv.close()
    n = g.tree.n_nodes
    order = np.argsort(par[1:], kind="stable") + 1                  # children of a node, ascending
    coff = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(par[1:], minlength=n), out=coff[1:])
    memo = {}

    def stack(k):
        """stack_muts of haplotype k (arena.cpp:17-48): the deepest mutation of the root path wins, back to the reference drops out"""
        s = memo.get(k)
        if s is None:
            seen, x = {}, k
            while True:
                for wd in words[int(woff[x]):int(woff[x + 1])].tolist():
                    p = wd & 0xFFFFF
                    if p not in seen:
                        seen[p] = None if ((wd >> 26) & 15) == (1 << ((wd >> 20) & 3)) else (wd >> 26) & 15
                if x == 0:
                    break
                x = int(par[x])
            s = memo[k] = sorted((p, m) for p, m in seen.items() if m is not None)
        return s

    out = {}
    for K, radius in CONFIGS:
        rows = []
        for target in pivots[K][: a.cpu_pivots].tolist():
            memo.clear()
            t0 = time.perf_counter()
            found, probes, q = set(), 0, deque([target])
            while q and probes < a.cpu_max_visits:                  # arena.cpp:171-198
                curr = q.popleft()
                if curr in found:
                    continue
                probes += 1
                d = mutation_distance(stack(curr), stack(target)) if a.form == w.NBR_TO_PIVOT else mutation_distance(stack(target), stack(curr))
                if d > radius:
                    continue
                found.add(curr)
                if curr:
                    q.append(int(par[curr]))
                q.extend(order[int(coff[curr]):int(coff[curr + 1])].tolist())
            rows.append({"pivot": target, "seconds": time.perf_counter() - t0, "probes": probes, "listed": len(found), "stopped": bool(q)})
        out["%d:%d" % (K, radius)] = rows
    json.dump({"host": platform.processor() or platform.machine(), "cpus": os.cpu_count(), "configs": out}, open(path, "w"))


if a.cpu_leg:
    cpu_leg(a.cpu_leg)
    sys.exit(0)

if a.cpu_json:
    cpu = json.load(open(a.cpu_json))
elif a.cpu_pivots:
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "cpu.json")
        args = ["--nodes", str(a.nodes), "--configs", a.configs, "--form", str(a.form), "--cpu-pivots", str(a.cpu_pivots),
                "--cpu-max-visits", str(a.cpu_max_visits)] + ([] if a.p_hub is None else ["--p-hub", str(a.p_hub)])
        subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-leg", f] + args, check=True)
        cpu = json.load(open(f))
else:
    cpu = None


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


# ---- the device -----------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
g, pivots = workload()
t_gen = time.perf_counter() - t0
t0 = time.perf_counter()
mat = w.Mat(g.tree)
t_mat = time.perf_counter() - t0
shape = g.shape() if hasattr(g, "shape") else None
res = {"row": "epp_neighbors (closest_neighbors / highest_scoring_neighbors)", "nodes": mat.n_nodes, "p_hub": a.p_hub, "form": a.form,
       "max_position": int(mat.stats.max_position), "gen_s": t_gen, "mat_create_s": t_mat, "configs": []}
mat.epp_neighbors(pivots[CONFIGS[0][0]][:4], 1, a.form)              # warm-up (and the handle's dfs_end)
for K, radius in CONFIGS:
    piv = pivots[K]
    walls, phases = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        out = mat.epp_neighbors(piv, radius, a.form, want_lists=False)
        walls.append(time.perf_counter() - t0)
        phases.append(w.epp_neighbors_last_timing())
    sizes = np.diff(out["nbr_off"]).astype(np.int64)
    total = int(out["nbr_off"][-1])
    row = {"pivots": K, "radius": radius, "passes": -(-K // max(4, ((2 << 30) // ((mat.n_nodes + 1) * 8)) // 4 * 4)),
           "sizes_only": {"tables_ms": spread([p["tables_ms"] for p in phases]), "field_ms": spread([p["field_ms"] for p in phases]),
                          "region_ms": spread([p["region_ms"] for p in phases]), "wall_s": spread(walls)},
           "list_entries": total, "list_size": {"min": int(sizes.min()), "median": float(np.median(sizes)), "mean": float(sizes.mean()),
                                                "max": int(sizes.max())},
           "top_is_root": int((out["top"] == 0).sum())}
    if total <= a.max_list_entries:
        t0 = time.perf_counter()
        full = mat.epp_neighbors(piv, radius, a.form, nbr_capacity=total)
        row["with_lists"] = dict(w.epp_neighbors_last_timing(), wall_s=time.perf_counter() - t0)
        assert np.array_equal(full["nbr_off"], out["nbr_off"])
    else:
        row["with_lists"] = None                                     # (larger than --max-list-entries: sizes only)
    if cpu:
        rows = cpu["configs"].get("%d:%d" % (K, radius), [])
        if rows:
            secs, probes = sum(r["seconds"] for r in rows), sum(r["probes"] for r in rows)
            ok = all(r["stopped"] or r["listed"] == int(sizes[i]) for i, r in enumerate(rows))
            row["cpu_baseline"] = {"kind": "port", "host": cpu["host"], "pivots": len(rows), "seconds": secs, "probes": probes,
                                   "probes_per_s": probes / secs if secs else None, "stopped_early": sum(r["stopped"] for r in rows),
                                   "sample": "closest_neighbors restated in Python for the first pivots, one process, each BFS stopped after "
                                             "%d probes" % a.cpu_max_visits, "matches_gpu_where_complete": ok}
    res["configs"].append(row)
mat.close()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
