"""Builders of the kinds of reads the placement routes differently (wepp_amd/csrc/device_mat.hpp: the plan classes),
shared by the GPU tests that mix them in one batch."""
import numpy as np

from wepp_amd import Reads

GENOME = 29903


def genome_samples(g, seed, n, genome_len=GENOME, p_sub=0.001, p_n=0.002, p_iupac=0.0):
    """Whole-genome samples drawn from the generated tree's leaves (PLAN_SEED)."""
    return g.reads(seed, n, read_len=genome_len, amplicon_len=genome_len, amplicon_step=genome_len, p_substitution=p_sub,
                   p_n=p_n, p_iupac=p_iupac)


def long_reads(g, seed, n):
    """1.2 kb reads of a midnight-like amplicon scheme, noisy enough to list more than 32 entries (PLAN_WIN): the
    parameters of bench.py's long-read leg."""
    return g.reads(seed, n, read_len=1200, amplicon_len=1200, amplicon_step=1020, p_substitution=0.03, p_n=0.02)


def far_samples(rng, n, genome_len=GENOME):
    """Samples far from every node of any tree: 25 - 69 random positions, a fifth of them N, the others a random
    non-reference allele.  Their best score hardly beats the root's, so levels of hundreds of chunks can tie and the
    seed kernel hands them to its second pass (seed_kernels.hip: SeedHeavy)."""
    samples = []
    for _ in range(n):
        k = int(rng.integers(25, 70))
        pos = np.sort(rng.choice(np.arange(1, genome_len + 1), size=k, replace=False))
        ents = []
        for p in pos:
            ref = 1 << int(rng.integers(0, 4))
            if rng.random() < 0.2:
                ents.append((int(p), ref, 15, 1))
            else:
                a = 1 << int(rng.integers(0, 4))
                ents.append((int(p), ref, a if a != ref else (ref << 1 if ref < 8 else 1), 0))
        samples.append(ents)
    return Reads.from_lists(samples)


def hot_position_reads(tree, rng, n, hot=400, k_lo=2, k_hi=12):
    """Reads of k_lo .. k_hi entries at the `hot` most mutated positions of the tree, anywhere on the genome: many events
    at their positions in the tree-wide stream (PLAN_WALKC8 / PLAN_WALKC16: a wave per 64 events, or jobs).  Half
    concrete alleles, a fifth ambiguity codes, the rest N."""
    pos_all = np.asarray(tree.mut_pos)
    keep = pos_all >= 0
    counts = np.bincount(pos_all[keep])
    ref = np.zeros(counts.size, np.int64)
    ref[pos_all[keep]] = np.asarray(tree.mut_ref)[keep]
    top = np.sort(np.argsort(counts, kind="stable")[::-1][:hot])
    samples = []
    for _ in range(n):
        k = int(rng.integers(k_lo, k_hi + 1))
        ents = []
        for p in np.sort(rng.choice(top, size=k, replace=False)):
            u = rng.random()
            if u < 0.5:
                ents.append((int(p), int(ref[p]), 1 << int(rng.integers(0, 4)), 0))
            elif u < 0.7:
                ents.append((int(p), int(ref[p]), int(rng.integers(1, 15)), 0))
            else:
                ents.append((int(p), int(ref[p]), 15, 1))
        samples.append(ents)
    return Reads.from_lists(samples)


def empty_reads(n):
    return Reads(np.zeros(n + 1, np.uint32), np.zeros(0, np.uint32))


def concat(batches):
    """One batch of the reads of several, in order."""
    offs, base = [np.zeros(1, np.int64)], 0
    for b in batches:
        offs.append(b.read_off[1:].astype(np.int64) + base)
        base += int(b.read_off[-1])
    return Reads(np.concatenate(offs).astype(np.uint32), np.concatenate([b.read_word for b in batches]))


def take(reads, idx):
    """The reads `idx` of a batch, in that order (a permutation, a repetition, a sample)."""
    idx = np.asarray(idx, np.int64)
    off = reads.read_off.astype(np.int64)
    k = off[idx + 1] - off[idx]
    new_off = np.concatenate([[0], np.cumsum(k)])
    # the word of entry e of read idx[i] sits at off[idx[i]] + e
    src = np.repeat(off[idx] - new_off[:-1], k) + np.arange(int(new_off[-1]))
    return Reads(new_off.astype(np.uint32), reads.read_word[src])
