"""Python model of the seed bound (wepp_amd/csrc/seed_kernels.hip) over the arrays the flattener
builds: the chunks of the whole-tree stream, their signatures, and the lower bound a sample's hard entries give for
every node of a chunk.  Checked against the oracle's per-node scores in tests/test_seed_model.py.

And of what k_seed does with the bound (tests/seed_cases.py, tests/test_seed_cases.py): the byte H_T(C) of every chunk
and the chunks per level, the hit events of a chunk's groups of blocks, the chunks the kernel must and may evaluate,
the level at which a sample is handed to the second pass."""
import numpy as np

# restated from seed_kernels.hip, device_mat.hpp and flatmat.hpp; tests/test_seed_cases.py reads them there with a regex
SEED_HIT_CAP = 96              # hit events of a group a wave lists; one more: block by block
SEED_MAX_HARD = 255            # hard entries counted per chunk (byte counters)
SEED_HEAVY_LEVEL_MIN = 256     # a level of that many chunks hands the sample to the second pass
SEED_HEAVY_PARTS = 32          # workgroups per handed-over sample
SEED_HEAVY_CAP = 128           # handed-over samples per call
SEED_MAX_ENTRIES = 4096        # entries of a seeded sample
SEED_MIN_HARD = 3              # hard entries of a seeded sample (the product's default)
SEED_THREADS = 512
SEED_CHUNK_BLOCKS = 16         # the product's blocks per chunk
GROUP_BLOCKS = 32              # blocks whose events a wave scans together
SCAN_ROUND = 8 * 64            # events of one round of the scan
SLAB = 64                      # chunks of a level one wave takes at a time
W_PAD_POS = 0xFFFFF


def seed_h_words(chunks):
    return ((chunks + 63) & ~63) // 4


def seed_lds_bytes(bm_words, ent_cap, chunks):
    """seed_lds_bytes of seed_kernels.hip: bitmap | words | hard entries | byte counters | shared scalars | hit lists"""
    waves = SEED_THREADS // 64
    return (bm_words + ent_cap + (SEED_MAX_HARD + 1) + seed_h_words(chunks) + (16 + 3 * waves) + waves * 3 * SEED_HIT_CAP) * 4


class SeedModel:
    def __init__(self, fv):
        st = fv.stats
        self.nch = int(st.seed_chunks)
        self.stride = int(st.seed_chunk_blocks)
        self.max_pos = int(st.max_position)
        self.built = self.nch > 0
        if not self.built:
            return
        node0 = fv.get("blk_node0")                      # [NB + 1] of the whole-tree stream: local = global DFS index
        nb = len(node0) - 1
        self.chunk_lo = np.array([node0[min(nb, c * self.stride)] for c in range(self.nch + 1)], np.int64)
        sig = fv.get("seed_sig")
        self.row_words = len(sig) // (self.max_pos + 2)
        self.sig = sig.reshape(self.max_pos + 2, self.row_words)
        self.dfs2bfs = fv.get("dfs2bfs")
        self.bfs2dfs = np.zeros(len(self.dfs2bfs), np.int64)
        self.bfs2dfs[self.dfs2bfs] = np.arange(len(self.dfs2bfs))
        self.nb = nb
        self.blk_node0 = node0.astype(np.int64)
        self.blk_eoff = fv.get("blk_eoff").astype(np.int64)
        self.ev_pos = (fv.get("ev_word") & W_PAD_POS).astype(np.int64)
        self.cp_stride = int(fv.cp_stride)
        self.n_cp = len(fv.get("cp_off")) - 1
        self.bm_words = 1
        while self.bm_words < (self.max_pos >> 5) + 1:
            self.bm_words <<= 1
        c = np.arange(self.nch)
        self._word, self._shift = c >> 3, ((c & 7) * 4).astype(np.uint32)

    def chunk_of_dfs(self, d):
        return int(np.searchsorted(self.chunk_lo, d, side="right") - 1)

    def nibble(self, pos, c):
        return (int(self.sig[pos, c >> 3]) >> ((c & 7) * 4)) & 15

    def hard_entries(self, S):
        """(entries with a signature row, entries beyond the tree's last mutated position): not missing, alleles
        excluding the entry's own reference base"""
        inside, beyond = [], 0
        for (p, ref, a, missing) in S:
            if missing or (a & ref):
                continue
            if p <= self.max_pos:
                inside.append((p, a))
            else:
                beyond += 1
        return inside, beyond

    def lower_bounds(self, S, max_hard=255):
        """|T| - H_T(C) for every chunk C (T = the first max_hard hard entries inside the tree + all beyond it)"""
        inside, beyond = self.hard_entries(S)
        inside = inside[:max_hard]
        sT = len(inside) + beyond
        H = np.zeros(self.nch, np.int64)
        for (p, a) in inside:
            for c in range(self.nch):
                if self.nibble(p, c) & a:
                    H[c] += 1
        return sT - H

    # ---- what the kernel does with the bound ------------------------------------------------------------------------
    def chunk_of_bfs(self, j):
        return self.chunk_of_dfs(int(self.bfs2dfs[j]))

    def chunk_blocks(self, c):
        return c * self.stride, min(self.nb, (c + 1) * self.stride)

    def counts(self, S, max_hard=SEED_MAX_HARD):
        """(H, |T|, nh): the byte H_T(C) of every chunk over the first max_hard hard entries inside the tree -- the
        kernel keeps an arbitrary max_hard of them when there are more --, |T| = nh + the hard entries beyond it"""
        inside, beyond = self.hard_entries(S)
        inside = inside[:max_hard]
        H = np.zeros(self.nch, np.int64)
        for (p, a) in inside:
            H += (((self.sig[p, self._word] >> self._shift) & 15 & a) != 0)
        return H, len(inside) + beyond, len(inside)

    def levels(self, S):
        """(H per chunk, chunks per level [256])"""
        H = self.counts(S)[0]
        return H, np.bincount(H, minlength=256)

    def defer_level(self, S):
        """The first level, from the largest count down, that holds SEED_HEAVY_LEVEL_MIN chunks or more; None: none"""
        H, cnt = self.levels(S)
        for h in range(int(H.max()), -1, -1):
            if cnt[h] >= SEED_HEAVY_LEVEL_MIN:
                return h
        return None

    def must_may(self, S, best, root_score):
        """must: chunks with |T| - H <= best -- every one of them is evaluated, whatever the order of the waves (the
        bound B never falls below the optimum); may: chunks with |T| - H <= root_score + 1 -- B starts there, nothing
        outside them can be evaluated."""
        H, sT, _ = self.counts(S)
        return int((sT - H <= best).sum()), int((sT - H <= root_score + 1).sum())

    def settled_at_the_top(self, S, best, best_bfs):
        """True when an optimal node lies in a chunk of the top level.  The levels are entered one after the other,
        behind a barrier, with the bound the levels above left: after the top level it is the optimum, so exactly the
        `must` chunks are evaluated.  (Not when the top level itself goes to the second pass on a tree of more chunks
        than one part takes: the parts share the bound without a barrier between them.)"""
        H = self.counts(S)[0]
        if self.defer_level(S) == int(H.max()) and self.nch > SLAB * (SEED_THREADS // 64):
            return False
        return any(H[self.chunk_of_bfs(j)] == H.max() for j in best_bfs)

    def group_hits(self, S, c):
        """Chunk c as a wave scans it: per group of up to GROUP_BLOCKS blocks, dict(blocks, events -- slots, padding
        included --, hits, per_block, rounds = hits per SCAN_ROUND slots).  A slot is a hit when the sample lists its
        position (an entry beyond max_pos sets no bit of the map, and no event sits there)."""
        pos = np.array(sorted(set(p for (p, _, _, _) in S if p <= self.max_pos)), np.int64)
        b0, b1 = self.chunk_blocks(c)
        out = []
        for bg in range(b0, b1, GROUP_BLOCKS):
            ng = min(GROUP_BLOCKS, b1 - bg)
            e0, e1 = int(self.blk_eoff[bg]), int(self.blk_eoff[bg + ng])
            hit = np.isin(self.ev_pos[e0:e1], pos)
            per_block = [int(hit[self.blk_eoff[bg + j] - e0:self.blk_eoff[bg + j + 1] - e0].sum()) for j in range(ng)]
            rounds = [int(hit[i:i + SCAN_ROUND].sum()) for i in range(0, e1 - e0, SCAN_ROUND)]
            out.append(dict(blocks=ng, events=e1 - e0, hits=int(hit.sum()), per_block=per_block, rounds=rounds))
        return out
