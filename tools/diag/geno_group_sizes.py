#!/usr/bin/env python3
"""How large do the groups of wepp_geno_diameters get?  CPU only: the synthetic tree of the bench (generate_tree(21,
--nodes)), ARTIC-like reads (--reads of 150 bases on amplicons of 400 every 300 sites), a mask that uncovers a fifth
of the genome (every fifth block of --mask-block sites), site_read_map and create_condensed_tree restated on arrays
(a node keeps the mutations at covered sites; a node left without one joins its nearest kept ancestor).  Prints (and
with --out writes) the histogram of sources per condensed node and the pairs their diameters take."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import wepp_amd as w

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--reads", type=int, default=200_000)
ap.add_argument("--mask-block", type=int, default=600)
ap.add_argument("--out")
a = ap.parse_args()

g = w.generate_tree(21, a.nodes)
t = g.tree
G = 29903
rd = g.reads(22, a.reads, windows=True)
cover = np.zeros(G + 2, np.int64)
np.add.at(cover, rd.start, 1)
np.add.at(cover, rd.end + 1, -1)
cover = np.cumsum(cover)[: G + 1]
pos, _, mut, _ = w.unpack_read_word(rd.read_word)
np.subtract.at(cover, pos[mut == 15], 1)                    # an N covers nothing
masked = (np.arange(G + 1) // a.mask_block) % 5 == 0
covered = (cover > 0) & ~masked
covered[0] = False
has = np.zeros(t.n_nodes, bool)
node_of = np.repeat(np.arange(t.n_nodes), np.diff(t.mut_off.astype(np.int64)))
ok = t.mut_pos >= 0
has[node_of[ok][covered[t.mut_pos[ok]]]] = True
parent = t.parent
assert (parent[1:] < np.arange(1, t.n_nodes)).all(), "a parent's id is smaller than its children's"
rep = np.arange(t.n_nodes)
for i in range(1, t.n_nodes):
    if not has[i]:
        rep[i] = rep[parent[i]]
sizes = np.bincount(rep)[np.unique(rep)]
edges = [1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513, 1025, 4097, 16385, 1 << 62]
hist = {("%d" % lo if hi == lo + 1 else "%d-%d" % (lo, hi - 1) if hi < 1 << 62 else ">=%d" % lo): int(((sizes >= lo) & (sizes < hi)).sum())
        for lo, hi in zip(edges[:-1], edges[1:])}
res = {"nodes": t.n_nodes, "reads": a.reads, "covered_sites": int(covered.sum()), "masked_sites": int(masked[1:].sum()), "condensed_nodes": int(sizes.size),
       "sources_per_condensed_node": hist, "largest": int(sizes.max()), "root_group": int(sizes[0] if rep[0] == 0 else 0),
       "pairs_all_groups": int((sizes.astype(np.int64) * (sizes - 1) // 2).sum()), "pairs_in_groups_above_64": int((sizes[sizes > 64].astype(np.int64) * (sizes[sizes > 64] - 1) // 2).sum()),
       "pairs_without_largest": int((np.sort(sizes)[:-1].astype(np.int64) * (np.sort(sizes)[:-1] - 1) // 2).sum())}
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
