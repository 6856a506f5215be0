#!/usr/bin/env python3
"""Measurement of wepp_epp_resolve (arena::resolve_unaccounted_mutations, src/WEPP/arena.cpp:739-892): N-node synthetic
MAT, R amplicon reads with windows, K haplotypes drawn with a seed, M residual mutations -- half of them alleles the reads
list, half the reference base at sites the reads cover, in a shuffled order.  A warm-up, then --steps calls; prints (and
with --out writes) one JSON object: the device time by phase (wepp_epp_resolve_last_timing, HIP events: mark, tables,
assign, tally) with its spread over the calls, mark and tally against the assignment of the same call, the bytes of tie
masks the tally reads, and the CPU loop the call replaces -- tests/resolve_model.py, the sequential Python restatement of
arena.cpp:746-892, on the first --cpu-reads reads in one host process (kind: "port"), compared with the device's
result on the same reads.

The CPU leg runs first, in a child process of its own that never opens the GPU (`--cpu-leg FILE` is that child)."""
import argparse, json, os, statistics, subprocess, sys, tempfile, time
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
ap.add_argument("--residual", type=int, default=500)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--cpu-reads", type=int, default=2000)
ap.add_argument("--out")
ap.add_argument("--cpu-leg")
a = ap.parse_args()


def workload():
    g = w.generate_tree(21, a.nodes)
    amp = max(400, a.read_len)
    reads = g.reads(22, a.reads, read_len=a.read_len, amplicon_len=amp, amplicon_step=300 if a.read_len < 400 else 1000,
                    windows=True, max_degree=5)
    rng = np.random.default_rng(23)
    sel = rng.permutation(g.tree.n_nodes)[: a.sel].astype(np.uint32)
    # the reference base where the tree or the reads tell it, A elsewhere (the call compares ref_nuc with mut_nuc only)
    ref = np.ones(GENOME + 2, np.uint32)
    t = g.tree
    ok = (t.mut_pos > 0) & (t.mut_pos <= GENOME) & np.isin(t.mut_ref, (1, 2, 4, 8))
    ref[t.mut_pos[ok]] = t.mut_ref[ok]
    pos, rf, mut, _ = w.unpack_read_word(reads.read_word)
    ok = (pos <= GENOME) & np.isin(rf, (1, 2, 4, 8))
    ref[pos[ok]] = rf[ok]
    n_alleles = a.residual // 2
    real = np.flatnonzero((mut != 15) & (pos <= GENOME))
    pick = rng.choice(real, size=min(n_alleles, real.size), replace=False) if real.size else np.zeros(0, np.int64)
    triples = {(int(pos[j]), int(ref[pos[j]]), int(mut[j])) for j in pick}
    while len(triples) < a.residual:                       # the reference base at a site some read covers
        r = int(rng.integers(0, reads.n_reads))
        p = int(rng.integers(int(reads.start[r]), min(int(reads.end[r]), GENOME) + 1))
        triples.add((p, int(ref[p]), int(ref[p])))
    triples = sorted(triples)
    rng.shuffle(triples)
    residual = np.array([int(w.pack_read_word(p, r, m)) for p, r, m in triples], np.uint32)
    return g, reads, sel, residual


def head(reads, n):
    return reads.__class__(reads.read_off[: n + 1], reads.read_word[: int(reads.read_off[n])], reads.start[:n], reads.end[:n],
                           reads.degree[:n])


KEYS = ("rel_off", "rel_read", "n_covered", "n_masked", "best_degree", "best_mask", "hap_reads", "hap_degree")

if a.cpu_leg:
    import resolve_model
    g, reads, sel, residual = workload()
    n = min(a.cpu_reads, reads.n_reads)
    import assign_model
    tab = assign_model.SelectionTable(g.tree, sel)
    t0 = time.perf_counter()
    out = resolve_model.resolve(g.tree, head(reads, n), GENOME, sel, residual, table=tab)
    dt = time.perf_counter() - t0
    np.savez(a.cpu_leg, n=n, seconds=dt, n_touched=out["n_touched"], **{k: out[k] for k in KEYS})
    sys.exit(0)

cpu = None
td = tempfile.TemporaryDirectory()
if a.cpu_reads:
    f = os.path.join(td.name, "cpu.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-leg", f] +
                   [x for k in ("nodes", "reads", "read_len", "sel", "residual", "cpu_reads")
                    for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))], check=True)
    cpu = np.load(f)

# ---- the device -----------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
g, reads, sel, residual = workload()
t_gen = time.perf_counter() - t0
t0 = time.perf_counter()
mat = w.Mat(g.tree)
t_mat = time.perf_counter() - t0
mat.epp_resolve(head(reads, 64), GENOME, sel, residual)       # warm-up
walls, phases = [], []
cap = None
for _ in range(a.steps):
    t0 = time.perf_counter()
    out = mat.epp_resolve(reads, GENOME, sel, residual, rel_capacity=cap)
    walls.append(time.perf_counter() - t0)
    phases.append(w.epp_resolve_last_timing())
    cap = int(out["rel_off"][-1])                              # (the first call may have run twice: its wall time says so)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


med = {k: statistics.median(p[k] for p in phases) for k in phases[0]}
slabs = (a.sel + 255) // 256
relations = int(out["rel_off"][-1])
res = {"row": "epp_resolve (resolve_unaccounted_mutations)", "nodes": mat.n_nodes, "reads": reads.n_reads, "read_len": a.read_len,
       "selected": a.sel, "residual": int(residual.size), "touched_reads": out["n_touched"], "relations": relations,
       "longest_relation_list": int(np.diff(out["rel_off"]).max()) if residual.size else 0,
       "mark_ms": spread([p["mark_ms"] for p in phases]), "tables_ms": spread([p["tables_ms"] for p in phases]),
       "assign_ms": spread([p["assign_ms"] for p in phases]), "tally_ms": spread([p["tally_ms"] for p in phases]),
       "wall_s": spread(walls), "mark_over_assign": med["mark_ms"] / med["assign_ms"] if med["assign_ms"] else None,
       "tally_over_assign": med["tally_ms"] / med["assign_ms"] if med["assign_ms"] else None,
       "tally_tie_mask_bytes": relations * slabs * 32,
       "tally_tie_mask_GBps": relations * slabs * 32 / (med["tally_ms"] / 1e3) / 1e9 if med["tally_ms"] else None,
       "reads_per_s_device": reads.n_reads / (sum(med.values()) / 1e3), "reads_per_s_wall": reads.n_reads / statistics.median(walls),
       "gen_s": t_gen, "mat_create_s": t_mat}
if cpu is not None:
    n = int(cpu["n"])
    got = mat.epp_resolve(head(reads, n), GENOME, sel, residual, want_tallies=True)
    ok = all(np.array_equal(np.asarray(got[k]), cpu[k]) for k in KEYS) and int(got["n_touched"]) == int(cpu["n_touched"])
    res["cpu_baseline"] = {"value": n / float(cpu["seconds"]), "unit": "reads/s", "cores": 1, "kind": "port",
                           "sample": f"first {n} reads x {a.sel} haplotypes x {int(residual.size)} residual mutations, arena.cpp:746-892 "
                                     "restated in Python (tests/resolve_model.py), the genotype table built beforehand",
                           "matches_gpu": bool(ok)}
mat.close()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
