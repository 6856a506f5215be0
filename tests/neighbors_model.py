"""Model of wepp_epp_neighbors: arena::closest_neighbors and arena::highest_scoring_neighbors
(src/WEPP/arena.cpp:171-249) restated literally -- stack_muts per haplotype as arena::from_mat builds them
(arena.cpp:17-48), haplotype::mutation_distance as a merge of two sorted lists (haplotype.hpp:123-181), the BFS
over parent and children, and the climb followed by the pruned DFS.  No path sums, no tables: what the kernels
(neighbors_kernels.hip) compute another way.  Haplotypes are arena (pre-order) indices.  Masked mutations carry no
position; they are left out of stack_muts, as the flattened tree leaves them out of its words."""
from collections import deque

import numpy as np

import fuzz_trees as ft
import wepp_amd as w

TO, FROM = w.NBR_TO_PIVOT, w.NBR_FROM_PIVOT
INT_MAX = 2**31 - 1


def mutation_distance(this, comp, min_pos=0, max_pos=INT_MAX):
    """haplotype::mutation_distance(comp, min_pos, max_pos) of the haplotype with stack_muts `this`; both are
    position-sorted lists of (position, mut_nuc)."""
    muts = 0
    i = 0
    while i < len(this) and this[i][0] < min_pos:
        i += 1
    last_i = i
    while last_i < len(this) and this[last_i][0] <= max_pos:
        last_i += 1
    j = 0
    while i < last_i or j < len(comp):
        if i == last_i:
            if comp[j][1] != 15:
                muts += 1
            j += 1
        elif j == len(comp):
            muts += 1
            i += 1
        elif this[i][0] < comp[j][0]:
            muts += 1
            i += 1
        elif this[i][0] > comp[j][0]:
            if comp[j][1] != 15:
                muts += 1
            j += 1
        elif this[i][1] != comp[j][1] and comp[j][1] != 15:
            muts += 1
            i += 1; j += 1
        else:
            i += 1; j += 1
    return muts


class Arena:
    """parent / children / stack_muts of every haplotype, by arena index"""

    def __init__(self, tree):
        fv = w.FlatView(tree)
        par, ids = fv.get("parent_dfs").copy(), fv.get("dfs2id").copy()
        fv.close()
        n = tree.n_nodes
        self.n = n
        self.parent = [-1] + [int(par[k]) for k in range(1, n)]
        self.children = [[] for _ in range(n)]
        for k in range(1, n):
            self.children[self.parent[k]].append(k)
        self.ref = {}
        self.stack = []
        for k in range(n):                                  # pre-order: a parent comes first
            i = int(ids[k])
            own = [(int(tree.mut_pos[m]), int(tree.mut_ref[m]), int(tree.mut_mut[m]))
                   for m in range(int(tree.mut_off[i]), int(tree.mut_off[i + 1])) if int(tree.mut_pos[m]) >= 0]
            for p, r, _ in own:
                self.ref[p] = r
            named = {p for p, _, _ in own}
            s = [m for m in self.stack[self.parent[k]] if m[0] not in named] if k else []
            s += [(p, mut) for p, r, mut in own if r != mut]    # (maybe rewound back to the original)
            self.stack.append(sorted(s))

    def dist(self, form, piv, node):
        if form == TO:
            return mutation_distance(self.stack[node], self.stack[piv])
        return mutation_distance(self.stack[piv], self.stack[node])

    def field(self, piv, form):
        return np.array([self.dist(form, piv, k) for k in range(self.n)], np.int32)

    def closest_neighbors(self, target, max_radius):
        """arena.cpp:171-198: {node: distance} of all_neighbors, before the ranking"""
        found = {}
        q = deque([target])
        while q:
            curr = q.popleft()
            if curr in found:
                continue
            d = mutation_distance(self.stack[curr], self.stack[target])
            if d > max_radius:
                continue
            found[curr] = d
            if self.parent[curr] >= 0:
                q.append(self.parent[curr])
            q.extend(self.children[curr])
        return found

    def possible_neighbors(self, pivot, max_radius):
        """arena.cpp:211-239 with include_mapped = true: {node: distance}"""
        curr = pivot
        while self.parent[curr] >= 0 and mutation_distance(self.stack[pivot], self.stack[self.parent[curr]]) <= max_radius:
            curr = self.parent[curr]
        found = {}
        todo = [curr]                                        # (the recursion, as a stack)
        while todo:
            x = todo.pop()
            d = mutation_distance(self.stack[pivot], self.stack[x])
            if d > max_radius:
                continue
            found[x] = d
            todo.extend(self.children[x])
        return found

    def region(self, piv, radius, form):
        return self.closest_neighbors(piv, radius) if form == TO else self.possible_neighbors(piv, radius)

    def neighbors(self, pivots, radius, form, skip=None):
        """what Mat.epp_neighbors returns"""
        off, nodes, dists, top, nreg = [0], [], [], [], []
        for p in pivots:
            reg = self.region(int(p), radius, form)
            top.append(min(reg))                             # (a component's highest node comes first in pre-order)
            nreg.append(len(reg))
            keep = sorted(k for k in reg if skip is None or not skip[k])
            nodes += keep
            dists += [reg[k] for k in keep]
            off.append(len(nodes))
        return dict(nbr_off=np.array(off, np.uint64), nbr_node=np.array(nodes, np.uint32), nbr_dist=np.array(dists, np.int32),
                    top=np.array(top, np.uint32), n_region=np.array(nreg, np.uint32))


def check_equal(got, want, tag=""):
    for k in ("nbr_off", "nbr_node", "nbr_dist", "top", "n_region"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (tag, k)


def hub_leaf(arena):
    """a leaf under the node with the most children (None: the tree is a single node)"""
    hub = max(range(arena.n), key=lambda k: len(arena.children[k]))
    leaves = [c for c in arena.children[hub] if not arena.children[c]]
    return leaves[-1] if leaves else (arena.n - 1 if arena.n > 1 else None)


def random_tree_with_n(rng, genome=60, max_muts=2, p_n=0.15, p_back=0.15):
    """fuzz_trees.random_tree never draws the allele N (15), the one place where the two forms of the distance
    differ: the same recipe with N alleles and more back-mutations (true parent alleles, positions that collide)"""
    n = int(rng.integers(2, 65))
    ref = {p: 1 << int(rng.integers(0, 4)) for p in range(1, genome + 1)}
    parent, geno, muts = [-1], [dict() for _ in range(n)], []
    for i in range(1, n):
        parent.append(int(rng.integers(0, i)))
    for i in range(n):
        g = dict(geno[parent[i]]) if i else {}
        ml = []
        for p in sorted(set(int(x) for x in rng.integers(1, genome + 1, size=int(rng.integers(0, max_muts + 1))))):
            cur = g.get(p, ref[p])
            while True:
                u = rng.random()
                m = 15 if u < p_n else ref[p] if u < p_n + p_back else 1 << int(rng.integers(0, 4))
                if m != cur:
                    break
            ml.append((p, ref[p], cur, m))
            g[p] = m
        geno[i] = g
        muts.append(ml)
    return w.Tree.from_lists(parent, muts)


FUZZ_SEED, FUZZ_TREES, FUZZ_RADII = 1717, 40, (0, 1, 2, 3)


def fuzz_cases(n_trees=FUZZ_TREES, seed=FUZZ_SEED):
    """(tree, arena, pivots) of the fuzz: the root, the last node in pre-order (its subtree ends at row N), a leaf
    under a hub and a few more.  At most two mutations per node keep neighbours within the small radii."""
    rng = np.random.default_rng(seed)
    for it in range(n_trees):
        tree = ft.random_tree(rng, genome=60, max_muts=2)[0] if it % 2 == 0 else random_tree_with_n(rng)
        ar = Arena(tree)
        piv = [0, ar.n - 1]
        h = hub_leaf(ar)
        if h is not None:
            piv.append(h)
        piv += [int(x) for x in rng.integers(0, ar.n, size=4)]
        seen = []
        for p in piv:
            if p not in seen:
                seen.append(p)
        yield tree, ar, np.array(seen, np.uint32)


def hand_cases():
    """name -> (tree, pivots, radius, skip, {form: lists per pivot}): small trees whose regions are known by hand
    (arena indices = the order of the lists here: every child follows its parent, siblings in order)"""
    A, C, N = w.A, w.C, w.N
    cases = {}
    # the pivot (1) has N where its sibling (2) and the root are reference: nodes cost nothing against the pivot's
    # N, the pivot's N costs one against every node that does not list the position
    t = w.Tree.from_lists([-1, 0, 0], [[], [(5, A, A, N)], []])
    cases["n_pivot"] = (t, [1], 0, None, {TO: [[0, 1, 2]], FROM: [[1]]})
    # 1 mutates 7, its child 2 takes it back: 2 has the root's genotype but lies behind 1
    t = w.Tree.from_lists([-1, 0, 1, 0], [[], [(7, A, A, C)], [(7, A, C, A)], []])
    cases["back_mutation_behind_a_bad_node"] = (t, [0, 2], 0, None, {TO: [[0, 3], [2]], FROM: [[0, 3], [2]]})
    # a chain of equal genotypes: the skipped middle is walked through
    t = w.Tree.from_lists([-1, 0, 1], [[(3, A, A, C)], [], []])
    cases["skip"] = (t, [0, 1], 0, [0, 1, 0], {TO: [[0, 2], [0, 2]], FROM: [[0, 2], [0, 2]]})
    return cases
