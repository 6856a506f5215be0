"""NumPy model of wepp_epp_assign (assign_kernels.hip): the selection's genotype table built from the
flattened tree exactly as k_assign_geno builds it (walk parent_dfs from the haplotype to the root over
node_woff / words, the deepest mutation at a position wins, kept when mut != ref), prefix counts down the
columns, the closed form of haplotype::mutation_distance (src/WEPP/haplotype.hpp:123-173), ties,
per-haplotype counts and coverage bitmaps (src/WEPP/arena.cpp:612-665)."""
import numpy as np

import wepp_amd as w


class SelectionTable:
    """geno[p, k] = allele mask of haplotype sel[k] at position p (0 = reference), pre[p, k] = its
    non-reference positions <= p, for p = 0 .. max_pos of the tree."""

    def __init__(self, tree, sel, flat=None):
        fv = flat if flat is not None else w.FlatView(tree)
        words, woff, par = fv.get("words"), fv.get("node_woff"), fv.get("parent_dfs")
        self.sel = np.ascontiguousarray(sel, dtype=np.uint32)
        self.max_pos = max(int(fv.get("maxnest").size), 1) - 1
        K = self.sel.size
        geno = np.zeros((self.max_pos + 1, K), np.uint8)
        for k in range(K):
            n = int(self.sel[k])
            while True:
                ws = words[int(woff[n]):int(woff[n + 1])]
                if ws.size:
                    p = (ws & 0xFFFFF).astype(np.int64)
                    mut = ((ws >> 26) & 15).astype(np.uint8)
                    ref = (1 << ((ws >> 20) & 3)).astype(np.uint8)
                    free = geno[p, k] == 0                     # (a node names a position once)
                    geno[p[free], k] = 0x80 | np.where(mut == ref, 0, mut)[free]
                if n == 0:
                    break
                n = int(par[n])
        self.geno = geno & 15
        self.pre = np.cumsum(self.geno != 0, axis=0, dtype=np.int32)
        if flat is None:
            fv.close()

    def distances(self, pos, mut, start, end):
        """d(read, k) for every selected haplotype: the closed form the kernel uses."""
        pos = np.asarray(pos, np.int64); mut = np.asarray(mut, np.int64)
        real = mut != 15
        d = self.pre[min(end, self.max_pos)] - self.pre[min(start - 1, self.max_pos)] + int(real.sum())
        inw = (pos >= start) & (pos <= end) & (pos <= self.max_pos)
        if inw.any():
            g = self.geno[pos[inw]].astype(np.int64)
            nz = g != 0
            eq = (g == mut[inw][:, None]) & real[inw][:, None]
            d = d - (nz.astype(np.int64) + (nz & eq)).sum(axis=0)
        return d.astype(np.int32)


def assign_from_distances(dist_of_read, K, reads, genome_size):
    """Everything wepp_epp_assign delivers, from d(r, .) = dist_of_read(r): an int array over the K selected
    haplotypes (the model's table, or the oracle's epp_distance restricted to the selection)."""
    R = reads.n_reads
    W = (int(genome_size) + 31) // 32
    pos, _, mut, _ = w.unpack_read_word(reads.read_word)
    md = np.zeros(R, np.int32); ne = np.zeros(R, np.uint32)
    off = np.zeros(R + 1, np.uint64)
    lists = []
    sel_reads = np.zeros(K, np.uint32); sel_degree = np.zeros(K, np.int64)
    cover = np.zeros((K, W), np.uint32)
    for r in range(R):
        a, b = int(reads.read_off[r]), int(reads.read_off[r + 1])
        s, e = int(reads.start[r]), int(reads.end[r])
        d = np.asarray(dist_of_read(r))
        md[r] = d.min()
        ties = np.flatnonzero(d == md[r])
        ne[r] = ties.size
        lists.append(ties.astype(np.uint32))
        off[r + 1] = off[r] + np.uint64(ties.size)
        sel_reads[ties] += 1
        sel_degree[ties] += int(reads.degree[r])
        cs, ce = max(s, 1), min(e, int(genome_size))
        if cs <= ce:
            bits = np.zeros(W * 32, bool)
            bits[cs - 1:ce] = True
            pn = pos[a:b][mut[a:b] == 15].astype(np.int64)
            pn = pn[(pn >= cs) & (pn <= ce)]
            bits[pn - 1] = False
            words = np.packbits(bits, bitorder="little").view("<u4")
            w0, w1 = (cs - 1) >> 5, (ce - 1) >> 5
            cover[ties, w0:w1 + 1] |= words[w0:w1 + 1]
    covered = np.unpackbits(cover.view(np.uint8), axis=1).sum(axis=1).astype(np.uint32)
    return dict(min_dist=md, n_epp=ne, asg_off=off, asg_sel=np.concatenate(lists) if lists else np.zeros(0, np.uint32),
                sel_reads=sel_reads, sel_degree=sel_degree, sel_covered=covered, cover_bits=cover)


def assign(tree, reads, genome_size, sel, flat=None, table=None):
    """What Mat.epp_assign returns (with lists and bits), computed on the host from the model's table."""
    tab = table if table is not None else SelectionTable(tree, sel, flat)
    pos, _, mut, _ = w.unpack_read_word(reads.read_word)

    def dist(r):
        a, b = int(reads.read_off[r]), int(reads.read_off[r + 1])
        return tab.distances(pos[a:b], mut[a:b], int(reads.start[r]), int(reads.end[r]))
    return assign_from_distances(dist, tab.sel.size, reads, genome_size)


def oracle_distances(otree, reads):
    """[R, N] haplotype::mutation_distance of every read to every haplotype of the tree (OracleTree.epp_distance)"""
    pos, ref, mut, _ = w.unpack_read_word(reads.read_word)
    rows = []
    for r in range(reads.n_reads):
        a, b = int(reads.read_off[r]), int(reads.read_off[r + 1])
        rows.append(otree.epp_distance(pos[a:b], ref[a:b], mut[a:b], int(reads.start[r]), int(reads.end[r])))
    return np.array(rows, np.int32).reshape(reads.n_reads, -1)


def check_equal(got, want, tag="", bits=True):
    keys = ["min_dist", "n_epp", "asg_off", "asg_sel", "sel_reads", "sel_degree", "sel_covered"] + (["cover_bits"] if bits else [])
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (tag, k)
