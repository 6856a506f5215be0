#!/usr/bin/env python3
"""Measurement of wepp_clade_assign (usher_common.cpp:597-616 for a batch) on the bench tree (generate_tree(21, --nodes))
with --columns annotation columns of --clades lineage names on random nodes, for two inputs:
  default   --reads of the bench's default reads (150 bases, ARTIC-like amplicons)
  ties      --tie-reads short reads (two entries each) on a polytomy tree of its own: --groups hubs under the root,
            each a node with one mutation, 16 mutation-free sub-parents and 1 .. --max-ties leaves (log-uniform) that
            all carry the hub's second mutation; a read with a hub's two mutations has exactly the hub's leaves as
            parsimony-optimal nodes (the bench tree itself gives a read some tens of ties, never thousands)
For each: wepp_place_batch and wepp_best_nodes once (not timed here), then a warm-up and --runs calls of
wepp_clade_assign (host buffers in, host buffers out) -- wall time with its spread and the three device phases of
wepp_clade_last_timing.  Beside it --host-runs runs of a plain host restatement of :603-615 on --threads threads
(tools/diag/clades_host_ref.cpp, built here with g++ -O2: std::string names, a parent walk per pair and column,
std::sort); its best clades and run counts are compared with the device's.  It is what a caller without the device
would run, not the reference's code (which runs the loop on one thread per sample).
Prints (and with --out writes) one JSON object."""
import argparse, ctypes, json, os, statistics, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import wepp_amd as w

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=16_000_000)
ap.add_argument("--reads", type=int, default=20_000)
ap.add_argument("--tie-reads", type=int, default=2_000)
ap.add_argument("--groups", type=int, default=200)
ap.add_argument("--max-ties", type=int, default=100_000)
ap.add_argument("--columns", type=int, default=2)
ap.add_argument("--clades", type=int, default=3000)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--host-runs", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--out")
a = ap.parse_args()


def host_lib():
    src = os.path.join(ROOT, "tools", "diag", "clades_host_ref.cpp")
    out = os.path.join(ROOT, "tools", "diag", "_build", "libclades_host_ref.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", out])
    L = ctypes.CDLL(out)
    L.clades_host_ref.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 13 + [ctypes.c_uint32] + [ctypes.c_void_p] * 2
    return L


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


def p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def annotate(rng, N, C, K, candidates):
    """K names on 3 K of the candidate nodes per column; "UNDEFINED" (id K + 1) sorts behind every "L%07u" """
    clade_id = np.zeros((C, N), np.uint32)
    for c in range(C):
        nodes = rng.choice(candidates, size=min(candidates.size, K * 3), replace=False)
        clade_id[c, nodes] = rng.integers(1, K + 1, size=nodes.size, dtype=np.uint32)
    return clade_id, np.full(C, K + 1, np.uint32)


def tie_tree(rng, groups, max_ties, subs=16):
    sizes = np.exp(rng.uniform(0, np.log(max_ties), groups)).astype(np.int64)
    N = 1 + groups * (1 + subs) + int(sizes.sum())
    parent = np.full(N, -1, np.int32)
    n_mut = np.zeros(N, np.uint32)
    pos = np.zeros(N, np.int32)
    hub = 1 + np.arange(groups) * (1 + subs)
    parent[hub] = 0
    n_mut[hub] = 1
    pos[hub] = 10 + 2 * np.arange(groups)
    for k in range(subs):
        parent[hub + 1 + k] = hub
    first = 1 + groups * (1 + subs) + np.concatenate(([0], np.cumsum(sizes)[:-1]))
    grp = np.repeat(np.arange(groups), sizes)
    leaf = np.arange(1 + groups * (1 + subs), N)
    parent[leaf] = hub[grp] + 1 + (leaf - first[grp]) * 7 % subs
    n_mut[leaf] = 1
    pos[leaf] = 11 + 2 * grp
    has = n_mut > 0
    mut_off = np.concatenate(([0], np.cumsum(n_mut))).astype(np.uint32)
    m = int(has.sum())
    tree = w.Tree(parent, mut_off, pos[has], np.full(m, 1, np.uint8), np.where(pos[has] % 2 == 0, 2, 4).astype(np.uint8), np.full(m, 1, np.uint8))
    inner = np.flatnonzero(np.arange(N) < 1 + groups * (1 + subs))
    return tree, sizes, inner


def measure(name, tree, clade_id, undefined, reads, lib):
    N, C = tree.n_nodes, clade_id.shape[0]
    mat = w.Mat(tree)
    mat.set_clades(clade_id, undefined)
    pl = mat.place_batch(reads)
    off, nodes = mat.best_nodes_csr(reads, pl)
    pairs = int(off[-1])
    nb = pl.num_best
    got = mat.clade_assign(reads, pl, off, nodes)             # warm-up (sizes the histograms with a second call)
    cap = int(got[1][-1])
    wall, phases = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        got = mat.clade_assign(reads, pl, off, nodes, capacity=cap)
        wall.append((time.perf_counter() - t0) * 1e3)
        phases.append(w.clade_last_timing())
    one = dict(nodes=N, reads=reads.n_reads, pairs=pairs, runs_out=cap,
               num_best=dict(median=float(np.median(nb)), max=int(nb.max()), ones=int((nb == 1).sum())),
               wall_ms=spread(wall), phases_ms={k: spread([ph[k] for ph in phases]) for k in phases[0]},
               keys_per_s=pairs * C / (statistics.median(wall) * 1e-3))
    if lib is not None:
        R, K1 = reads.n_reads, int(undefined[0])
        is_leaf = np.ones(N, np.uint8)
        is_leaf[tree.parent[tree.parent >= 0]] = 0
        bfs2id = mat.bfs_order()
        hb = np.zeros((C, R), np.uint32); hr = np.zeros(C * R, np.uint32)
        rw = reads.read_word if reads.read_word.size else np.zeros(1, np.uint32)
        bj = np.ascontiguousarray(pl.best_bfs_j, np.uint32)
        hw = []
        for _ in range(a.host_runs):
            t0 = time.perf_counter()
            lib.clades_host_ref(N, R, C, p(tree.parent), p(tree.mut_off), p(tree.mut_pos), p(tree.mut_ref), p(tree.mut_mut), p(is_leaf),
                                p(bfs2id), p(reads.read_off), p(rw), p(bj), p(off), p(nodes), p(clade_id), a.threads, p(hb), p(hr))
            hw.append((time.perf_counter() - t0) * 1e3)
        hb[hb == 0] = K1
        same = bool(np.array_equal(hb, got[0]) and np.array_equal(hr, np.diff(got[1].astype(np.int64)).astype(np.uint32)))
        one["host"] = dict(wall_ms=spread(hw), same_best_and_run_counts=same)
        one["device_over_host"] = one["wall_ms"]["median"] / one["host"]["wall_ms"]["median"]
    mat.close()
    return one


rng = np.random.default_rng(5)
C, K = a.columns, a.clades
lib = host_lib() if a.host_runs else None
res = dict(kind="wepp_clade_assign", columns=C, clade_names=K, threads=a.threads, inputs={})
g = w.generate_tree(21, a.nodes)
cid, und = annotate(rng, g.tree.n_nodes, C, K, np.arange(g.tree.n_nodes))
reads = g.reads(22, a.reads, read_len=150, amplicon_len=400, amplicon_step=300, p_substitution=0.001, p_n=0.005)
res["inputs"]["default"] = measure("default", g.tree, cid, und, reads, lib)
del g, cid, reads
tt, sizes, inner = tie_tree(rng, a.groups, a.max_ties)
cid, und = annotate(rng, tt.n_nodes, C, 40, inner)
pick = rng.integers(0, a.groups, a.tie_reads)
words = np.empty(2 * a.tie_reads, np.uint32)
words[0::2] = w.pack_read_word(10 + 2 * pick, 1, 2)
words[1::2] = w.pack_read_word(11 + 2 * pick, 1, 4)
reads = w.Reads(np.arange(a.tie_reads + 1, dtype=np.uint32) * 2, words)
res["inputs"]["ties"] = measure("ties", tt, cid, und, reads, lib)
assert res["inputs"]["ties"]["pairs"] == int(sizes[pick].sum())
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
