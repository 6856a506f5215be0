#!/usr/bin/env python3
"""Measurement of wepp_epp_assign (arena::dump_read2haplotype_mapping, src/WEPP/arena.cpp:590-696): N-node synthetic
MAT, R amplicon reads with windows, K haplotypes drawn with a seed.  A warm-up, then --steps calls; prints (and with
--out writes) one JSON object: the device time by phase (wepp_epp_assign_last_timing, HIP events) with its spread
over the calls, reads/s, the bytes the table rows ask for, wepp_epp_map on the same reads for context, and the CPU
loop the call replaces -- a literal Python restatement of haplotype::mutation_distance (haplotype.hpp:123-173) and of
arena.cpp:612-625 on a bounded sample of the same reads, on --cpu-procs host processes (kind: "port").

The CPU leg runs first, in a child process of its own that never opens the GPU (`--cpu-leg FILE` is that child)."""
import argparse, bisect, json, multiprocessing, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wepp_amd as w

GENOME = 29903
ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--sel", type=int, default=512)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--cpu-reads", type=int, default=4000)
ap.add_argument("--cpu-procs", type=int, default=16)
ap.add_argument("--out")
ap.add_argument("--cpu-leg")
a = ap.parse_args()


def workload():
    g = w.generate_tree(21, a.nodes)
    amp = max(400, a.read_len)
    reads = g.reads(22, a.reads, read_len=a.read_len, amplicon_len=amp, amplicon_step=300 if a.read_len < 400 else 1000,
                    windows=True, max_degree=5)
    sel = np.random.default_rng(23).permutation(g.tree.n_nodes)[: a.sel].astype(np.uint32)
    return g, reads, sel


def head(reads, n):
    return reads.__class__(reads.read_off[: n + 1], reads.read_word[: int(reads.read_off[n])], reads.start[:n], reads.end[:n],
                           reads.degree[:n])


# ---- the CPU leg ---------------------------------------------------------------------------------------------
def mutation_distance(spos, smut, comp, min_pos, max_pos):
    """haplotype.hpp:123-173, line by line (stack_muts as two parallel lists, comp as (position, mut_nuc) pairs)"""
    muts = 0
    i = bisect.bisect_left(spos, min_pos)
    last_i = bisect.bisect_right(spos, max_pos)
    j = 0
    nc = len(comp)
    while i < last_i or j < nc:
        if i == last_i:
            if comp[j][1] != 15:
                muts += 1
            j += 1
        elif spos[i] < min_pos:
            i += 1
        elif spos[i] > max_pos:
            return muts
        elif j == nc:
            muts += 1; i += 1
        elif spos[i] < comp[j][0]:
            muts += 1; i += 1
        elif spos[i] > comp[j][0]:
            if comp[j][1] != 15:
                muts += 1
            j += 1
        elif smut[i] != comp[j][1] and comp[j][1] != 15:
            muts += 1; i += 1; j += 1
        else:
            i += 1; j += 1
    return muts


_HAPS = None


def _chunk(job):
    out = []
    for comp, s, e in job:
        epps, min_dist = [], 2**31 - 1                          # arena.cpp:614-625
        for k, (spos, smut) in enumerate(_HAPS):
            d = mutation_distance(spos, smut, comp, s, e)
            if d <= min_dist:
                if d < min_dist:
                    min_dist = d
                    epps = []
                epps.append(k)
        out.append((min_dist, len(epps)))
    return out


def cpu_leg(path):
    global _HAPS
    import assign_model
    g, reads, sel = workload()
    n = min(a.cpu_reads, reads.n_reads)
    tab = assign_model.SelectionTable(g.tree, sel)
    _HAPS = []
    for k in range(sel.size):
        p = np.flatnonzero(tab.geno[:, k])
        _HAPS.append((p.tolist(), tab.geno[p, k].tolist()))
    pos, _, mut, _ = w.unpack_read_word(reads.read_word)
    jobs = []
    for r in range(n):
        lo, hi = int(reads.read_off[r]), int(reads.read_off[r + 1])
        jobs.append((list(zip(pos[lo:hi].tolist(), mut[lo:hi].tolist())), int(reads.start[r]), int(reads.end[r])))
    per = max(1, n // (4 * a.cpu_procs))
    chunks = [jobs[i:i + per] for i in range(0, n, per)]
    with multiprocessing.get_context("fork").Pool(a.cpu_procs) as pool:      # (no GPU in this process: _HAPS is inherited)
        t0 = time.perf_counter()
        res = [x for c in pool.map(_chunk, chunks) for x in c]
        dt = time.perf_counter() - t0
    json.dump({"n": n, "seconds": dt, "min_dist": [x[0] for x in res], "n_epp": [x[1] for x in res]}, open(path, "w"))


if a.cpu_leg:
    cpu_leg(a.cpu_leg)
    sys.exit(0)

cpu = None
if a.cpu_reads:
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "cpu.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-leg", f] +
                       [x for k in ("nodes", "reads", "read_len", "sel", "cpu_reads", "cpu_procs")
                        for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))], check=True)
        cpu = json.load(open(f))

# ---- the device -----------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
g, reads, sel = workload()
t_gen = time.perf_counter() - t0
t0 = time.perf_counter()
mat = w.Mat(g.tree)
t_mat = time.perf_counter() - t0
mat.epp_assign(head(reads, 64), GENOME, sel)                    # warm-up
walls, phases = [], []
for _ in range(a.steps):
    t0 = time.perf_counter()
    out = mat.epp_assign(reads, GENOME, sel)
    walls.append(time.perf_counter() - t0)
    phases.append(w.epp_assign_last_timing())


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


# bytes the table rows ask for (algorithmic): per read and slab of 256 haplotypes two rows of prefix counts (512 B
# each) and one genotype row (256 B) per listed position inside the window and the tree's positions
pos = (reads.read_word & 0xFFFFF).astype(np.int64)
rid = np.repeat(np.arange(reads.n_reads), np.diff(reads.read_off).astype(np.int64))
max_pos = int(mat.stats.max_position)
inw = (pos >= reads.start[rid]) & (pos <= reads.end[rid]) & (pos <= max_pos)
slabs = (a.sel + 255) // 256
groups = (slabs + 3) // 4
passes = 1 if groups == 1 else 2                                # beyond 1024 haplotypes the distances are computed twice
row_bytes = passes * slabs * (2 * 512 * reads.n_reads + 256 * int(inw.sum()))
assign_ms = statistics.median(p["assign_ms"] for p in phases)
res = {"row": "epp_assign (dump_read2haplotype_mapping)", "nodes": mat.n_nodes, "reads": reads.n_reads, "read_len": a.read_len,
       "selected": a.sel, "max_position": max_pos,
       "tables_ms": spread([p["tables_ms"] for p in phases]), "assign_ms": spread([p["assign_ms"] for p in phases]),
       "finish_ms": spread([p["finish_ms"] for p in phases]), "wall_s": spread(walls),
       "reads_per_s_device": reads.n_reads / (statistics.median(sum(p.values()) for p in phases) / 1e3),
       "reads_per_s_wall": reads.n_reads / statistics.median(walls),
       "pairs_per_s_assign": reads.n_reads * a.sel / (assign_ms / 1e3),
       "table_row_bytes": row_bytes, "table_row_bytes_per_read": row_bytes / reads.n_reads,
       "table_row_GBps_assign": row_bytes / (assign_ms / 1e3) / 1e9,
       "table_bytes": (max_pos + 1) * slabs * 256 * 3,
       "mean_n_epp": float(out["n_epp"].mean()), "mean_min_dist": float(out["min_dist"].mean()),
       "list_entries": int(out["asg_off"][-1]), "gen_s": t_gen, "mat_create_s": t_mat}
t0 = time.perf_counter()
mat.epp_map(reads, GENOME, want_lists=False)
res["epp_map_same_reads"] = {"wall_s": time.perf_counter() - t0, "phases": w.epp_last_timing()}
if cpu:
    n = cpu["n"]
    ok = bool((np.array(cpu["min_dist"]) == out["min_dist"][:n]).all() and (np.array(cpu["n_epp"]) == out["n_epp"][:n]).all())
    res["cpu_baseline"] = {"value": n / cpu["seconds"], "unit": "reads/s", "cores": a.cpu_procs, "kind": "port",
                           "sample": f"first {n} reads x {a.sel} haplotypes, mutation_distance + arena.cpp:612-625 restated in Python, "
                                     f"{a.cpu_procs} processes", "matches_gpu": ok}
mat.close()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
