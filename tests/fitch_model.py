"""A plain 64-bit restatement of mapper_body (src/usher_mapper.cpp:7-162) in NumPy, vectorised over the rows of a
call: the second, independent expectation of the Fitch-Sankoff tests (the first is oracle/mapper2_oracle.c) and
their range guard.  The reference and the oracle add scores in `int`; a row whose exact scores reach 2^31 has no
defined answer, so every row a test uses must keep `max_score` below INT_LIMIT.

Rules, as the reference has them: a leaf starts at N for every base but the reference base; an observation sets
every base of its node to 0 (allowed) or N (not allowed), a later observation of the same node replacing an earlier
one; a child adds min(s[j], min_k s[k] + 1, N + 1) to base j of its parent; the backward pass keeps the parent's
state when it attains the minimum, else takes the lowest minimal base; mutations come out in row order, in BFS order
inside a row (children by ascending node id)."""
import numpy as np

INT_LIMIT = 2**31 - 1


class Topology:
    """BFS order (children by ascending id), levels, depth and child counts of a parent array with ids in any order."""

    def __init__(self, parent):
        parent = np.asarray(parent, np.int64)
        n = len(parent)
        roots = np.flatnonzero(parent < 0)
        assert len(roots) == 1, "one root"
        kids = np.flatnonzero(parent >= 0)
        kids = kids[np.argsort(parent[kids], kind="stable")]             # by parent, ascending id inside a parent
        n_children = np.bincount(parent[parent >= 0], minlength=n).astype(np.int64)
        child_off = np.zeros(n + 1, np.int64)
        np.cumsum(n_children, out=child_off[1:])
        level = roots
        bfs, level_off = [], [0]
        while len(level):
            bfs.append(level)
            level_off.append(level_off[-1] + len(level))
            cnt = n_children[level]
            tot = int(cnt.sum())
            if tot == 0:
                break
            # children of the level's nodes, node after node
            start = np.repeat(child_off[level] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
            level = kids[start + np.arange(tot)]
        self.n = n
        self.parent = parent
        self.bfs2id = np.concatenate(bfs)
        assert len(self.bfs2id) == n, "every node hangs under the root"
        self.id2bfs = np.empty(n, np.int64)
        self.id2bfs[self.bfs2id] = np.arange(n)
        self.level_off = np.array(level_off, np.int64)
        self.n_children = n_children                                      # by id
        self.max_children = int(n_children.max()) if n else 0
        self.max_depth = len(level_off) - 2                               # edges from the root to the deepest node
        self.is_leaf_bfs = n_children[self.bfs2id] == 0
        pb = np.zeros(n, np.int64)
        nonroot = self.bfs2id[1:]
        pb[1:] = self.id2bfs[parent[nonroot]]
        self.parent_bfs = pb
        self.level_nodes = np.diff(self.level_off)

    def depth_of_ids(self):
        d = np.zeros(self.n, np.int64)
        lev = np.repeat(np.arange(len(self.level_nodes)), self.level_nodes)
        d[self.bfs2id] = lev
        return d


def _last_entries(nodes, nucs):
    """of the entries that name the same node, the last one"""
    if len(nodes) == 0:
        return nodes, nucs
    rev = nodes[::-1]
    _, first = np.unique(rev, return_index=True)
    keep = len(nodes) - 1 - first
    return nodes[keep], nucs[keep]


def mapper_rows(topo, site_ref, var_off, var_node, var_nuc, block_bytes=1 << 29):
    """mapper_body on every row.  Returns (site, node id, par_nuc mask, mut_nuc mask) arrays in the reference's order
    and the largest score any row ever held."""
    if not isinstance(topo, Topology):
        topo = Topology(topo)
    n = topo.n
    site_ref = np.asarray(site_ref, np.int64)
    var_off = np.asarray(var_off, np.int64)
    var_node = np.asarray(var_node, np.int64)
    var_nuc = np.asarray(var_nuc, np.int64)
    rows = len(site_ref)
    ref_idx = np.zeros(rows, np.int64)
    for r in range(rows):
        m = int(site_ref[r])
        assert m in (1, 2, 4, 8), "site_ref is one base"
        ref_idx[r] = m.bit_length() - 1
    per_block = max(1, int(block_bytes // (n * 4 * 8 * 3)))
    out = [[], [], [], []]
    max_score = 0
    bases = np.arange(4)
    for r0 in range(0, rows, per_block):
        r1 = min(rows, r0 + per_block)
        R = r1 - r0
        S = np.zeros((R, n, 4), np.int64)
        leaf = np.flatnonzero(topo.is_leaf_bfs)
        for r in range(R):
            S[r, leaf[:, None], bases[None, :]] = np.where(bases == ref_idx[r0 + r], 0, n)[None, :]
            a, b = int(var_off[r0 + r]), int(var_off[r0 + r + 1])
            nodes, nucs = _last_entries(var_node[a:b], var_nuc[a:b])
            if len(nodes):
                S[r, topo.id2bfs[nodes], :] = np.where((nucs[:, None] >> bases[None, :]) & 1, 0, n)
        # forward pass, deepest level first: the children of a level's nodes are the next level, siblings together
        lo = topo.level_off
        for lev in range(len(lo) - 2, 0, -1):
            a, b = int(lo[lev]), int(lo[lev + 1])
            s = S[:, a:b, :]
            c = np.minimum(np.minimum(s, s.min(axis=2, keepdims=True) + 1), n + 1)
            pb = topo.parent_bfs[a:b]
            starts = np.flatnonzero(np.concatenate([[True], pb[1:] != pb[:-1]]))
            S[:, pb[starts], :] += np.add.reduceat(c, starts, axis=1)
        max_score = max(max_score, int(S.max()))
        # backward pass, root first
        state = np.zeros((R, n), np.int64)
        par_state = np.zeros((R, n), np.int64)
        for lev in range(len(lo) - 1):
            a, b = int(lo[lev]), int(lo[lev + 1])
            ps = np.broadcast_to(ref_idx[r0:r1, None], (R, 1)) if lev == 0 else state[:, topo.parent_bfs[a:b]]
            s = S[:, a:b, :]
            at_par = np.take_along_axis(s, ps[:, :, None], axis=2)[:, :, 0]
            state[:, a:b] = np.where(at_par == s.min(axis=2), ps, s.argmin(axis=2))
            par_state[:, a:b] = ps
        rr, bb = np.nonzero(state != par_state)                           # row-major: rows, then BFS index
        out[0].append((rr + r0).astype(np.uint32))
        out[1].append(topo.bfs2id[bb].astype(np.uint32))
        out[2].append((1 << par_state[rr, bb]).astype(np.uint8))
        out[3].append((1 << state[rr, bb]).astype(np.uint8))
    if rows == 0:
        return (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint8)), 0
    return tuple(np.concatenate(x) for x in out), max_score
