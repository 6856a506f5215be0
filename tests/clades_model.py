"""Literal Python restatement of the reference's clade assignment of a placed sample
(src/usher_common.cpp:603-615): per annotation column and optimal node, has_unique as
mapper2_body computes it (src/usher_mapper.cpp:191-262), Tree::get_clade_assignment as a walk up the parents
(src/mutation_annotated_tree.cpp:923-931), and Python's sort on the NAMES.  Nothing here knows about ids, tables
or the device: tests compare the C-ABI's numbers with what these strings give."""
import numpy as np


def tree_lists(tree):
    """(parent list, muts[node] = [(position, ref, par, mut)]) of a wepp_amd.Tree."""
    n = tree.n_nodes
    par = tree.mut_par if tree.mut_par is not None else tree.mut_ref
    muts = []
    for i in range(n):
        lo, hi = int(tree.mut_off[i]), int(tree.mut_off[i + 1])
        muts.append([(int(tree.mut_pos[k]), int(tree.mut_ref[k]), int(par[k]), int(tree.mut_mut[k])) for k in range(lo, hi)])
    return [int(p) for p in tree.parent], muts


def bfs_order(parent):
    """breadth_first_expansion (mutation_annotated_tree.cpp:1115-1141): children in ascending id."""
    n = len(parent)
    kids = [[] for _ in range(n)]
    root = 0
    for i, p in enumerate(parent):
        if p < 0:
            root = i
        else:
            kids[p].append(i)
    order = [root]
    for node in order:
        order.extend(kids[node])
    return order, kids


def has_unique(node_muts, is_root, sample):
    """usher_mapper.cpp:184-262.  sample = [(position, ref, mut, is_missing)] sorted by position."""
    unique = False
    if not is_root:                                              # :191
        start_index = 0
        for (p1, r1, _pa1, m1) in node_muts:                    # :193
            anc_nuc = m1
            if p1 < 0:                                           # :198 masked
                unique = True
                break
            found = False
            found_pos = False
            k = start_index
            while k < len(sample):                               # :205
                (p2, _r2, m2, miss2) = sample[k]
                start_index = k
                if p1 == p2:                                     # :208
                    found_pos = True
                    if miss2:                                    # :210
                        found = True
                    elif (m2 & anc_nuc) != 0:                    # :215
                        found = True
                        break
                if p1 < p2:                                      # :240
                    break
                k += 1
            if not found:                                        # :244
                if (not found_pos) and anc_nuc == r1:            # :245
                    pass
                else:
                    unique = True                                # :262
    return unique


def clade_assignment(parent, column, node, include_self):
    """Tree::get_clade_assignment: the first non-empty annotation on rsearch(node, include_self)."""
    cur = node if include_self else parent[node]
    while cur >= 0:
        if column[cur] != "":
            return column[cur]
        cur = parent[cur]
    return "UNDEFINED"


def assign_sample(parent, kids, muts, bfs, columns, sample, best_j_vec, best_j):
    """usher_common.cpp:603-615 for one sample: per column (best_clade_assignment, sorted clade_assignments), and the
    (node, include_self) of every pair."""
    pairs = []
    for j in best_j_vec:
        node = bfs[int(j)]
        is_leaf = not kids[node]
        unique = has_unique(muts[node], parent[node] < 0, sample)
        pairs.append((node, (not is_leaf) and (not unique), unique))      # :607
    out = []
    for column in columns:
        names = []
        best = None
        for (j, (node, include_self, _u)) in zip(best_j_vec, pairs):
            name = clade_assignment(parent, column, node, include_self)
            names.append(name)
            if int(j) == int(best_j):                                     # :610
                best = name
        names.sort()                                                      # :614
        out.append((best, names))
    return out, pairs


def run_lengths(names):
    """The -D writer's runs (usher_common.cpp:937-954): [(name, count)] of a sorted list."""
    runs = []
    for nm in names:
        if runs and runs[-1][0] == nm:
            runs[-1][1] += 1
        else:
            runs.append([nm, 1])
    return [(a, b) for a, b in runs]


def expected_arrays(per_sample, name_ids):
    """What wepp_clade_assign must deliver for a batch: per_sample[r] = assign_sample(...)[0], name_ids[c] = {name: id}.
    Returns (best_clade [C, R], hist_off, hist_clade, hist_count)."""
    R = len(per_sample)
    C = len(name_ids)
    best = np.zeros((C, R), np.uint32)
    off = [0]
    clade, count = [], []
    for c in range(C):
        for r in range(R):
            b, names = per_sample[r][c]
            best[c, r] = name_ids[c][b]
            for (nm, k) in run_lengths(names):
                clade.append(name_ids[c][nm])
                count.append(k)
            off.append(len(clade))
    return best, np.array(off, np.uint64), np.array(clade, np.uint32), np.array(count, np.uint32)


def format_clades_row(sample_name, per_column, detailed):
    """One row of clades.txt (usher_common.cpp:931-960)."""
    row = sample_name + "\t"
    for k, (best, names) in enumerate(per_column):
        row += best
        if detailed:
            row += "*|"
            row += ",".join("%s(%d/%d)" % (nm, cnt, len(names)) for (nm, cnt) in run_lengths(names))
        if k + 1 < len(per_column):
            row += "\t"
    return row + "\n"
