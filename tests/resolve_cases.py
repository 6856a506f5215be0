"""Inputs shared by the tests of wepp_epp_resolve (model, emulation, GPU): the hand cases of the three-way rule,
residual lists drawn so that every branch occurs, and relation lists of a given length."""
import numpy as np

import wepp_amd as w

GENOME = 60
Nn = lambda p, ref: (p, ref, w.N, 1)


def hand_tree():
    """reference: A everywhere but G at 40; haplotype 1 carries A5C, 2 adds G40T, 3 takes 5 back; the tree's last
    mutated position is 40"""
    tree = w.Tree.from_lists([-1, 0, 1, 1], [[], [(5, w.A, w.A, w.C)], [(40, w.G, w.G, w.T)], [(5, w.A, w.C, w.A)]])
    ref = {p: (w.G if p == 40 else w.A) for p in range(1, GENOME + 1)}
    return tree, ref


def hand_cases():
    """(name, tree, reads, genome, sel, residual) -- residual as (pos, ref, mut) in the caller's order"""
    tree, ref = hand_tree()
    out = []

    def case(name, reads, start, end, degree, residual, sels=([0, 1, 2, 3], [3, 1], [2])):
        rd = w.EppReads.from_lists(reads, start, end, degree)
        for sel in sels:
            out.append((f"{name}/sel={sel}", tree, rd, GENOME, np.array(sel, np.uint32), list(residual)))

    # two residual alleles at one position, both orders, against a read with entry C at p, N at p, nothing at p
    p = 10
    trio = [[(p, w.A, w.C)], [Nn(p, w.A)], [], [(p, w.A, w.T)]]
    for name, res in (("same-pos C,T", [(p, w.A, w.C), (p, w.A, w.T)]), ("same-pos T,C", [(p, w.A, w.T), (p, w.A, w.C)]),
                      ("same-pos ref,C", [(p, w.A, w.A), (p, w.A, w.C)]), ("same-pos C,ref", [(p, w.A, w.C), (p, w.A, w.A)]),
                      ("same-pos C,C|T", [(p, w.A, w.C), (p, w.A, w.C | w.T), (p, w.A, w.G)])):
        case(name, trio, [3, 3, 3, 8], [30, 30, 30, 12], [1, 2, 3, 4], res)
    # insertion before the first entry, between entries, after the last one, into a read with no entries
    ins = [[(20, w.A, w.C), (30, w.A, w.T)], [], [(5, w.A, w.C), (20, w.A, w.G)]]
    case("insert", ins, [2, 10, 1], [50, 50, 40], [1, 1, 5],
         [(35, w.A, w.A), (15, w.A, w.A), (25, w.A, w.A), (4, w.A, w.A), (40, w.G, w.G), (20, w.A, w.C)])
    # pos equal to start, end, start - 1, end + 1
    case("window", [[], [(20, w.A, w.C)], [(30, w.A, w.C)]], [20, 20, 21], [30, 30, 30], [1, 1, 1],
         [(20, w.A, w.A), (30, w.A, w.A), (19, w.A, w.A), (31, w.A, w.A), (20, w.A, w.C), (30, w.A, w.C)])
    # positions beyond the tree's last mutated position (40), a window that ends past the genome, a mutation no
    # read meets
    case("beyond", [[], [(55, w.A, w.T)], [Nn(57, w.A)]], [45, 50, 50], [58, 70, 60], [2, 1, 1],
         [(55, w.A, w.A), (55, w.A, w.T), (57, w.A, w.G), (60, w.A, w.A), (44, w.A, w.A), (41, w.A, w.C)])
    # every read of a mutation has degree 0: best holds the haplotypes that appeared, not all of the selection
    case("degree 0", [[(5, w.A, w.C)], [(5, w.A, w.C), (40, w.G, w.T)], [(5, w.A, w.C)]], [1, 1, 1], [45, 45, 45], [0, 0, 7],
         [(40, w.G, w.T), (20, w.A, w.A)], sels=([0, 1, 2, 3], [2, 0]))
    # the tally exceeds 2^32
    big = 2**31 - 1
    case("int64", [[(5, w.A, w.C)], [(5, w.A, w.C)], [(5, w.A, w.C)], []], [1, 1, 1, 1], [30, 30, 30, 30], [big, big, big, big],
         [(5, w.A, w.C), (12, w.A, w.A)])
    # the touched read that comes last (by index and in window order) ends with an inserted word that decides its ties:
    # N at 40 puts haplotype 2 (G40T) level with haplotype 1.  The end offset of the touched batch is this word's: one
    # word less and haplotype 2 drops out of best_mask
    case("last word", [[], [(5, w.A, w.C)]], [1, 1], [44, 45], [2, 3], [(40, w.G, w.G)], sels=([0, 1, 2, 3], [2, 1]))
    # no read is touched
    case("untouched", [[(5, w.A, w.C)], []], [1, 10], [30, 40], [1, 1], [(5, w.A, w.T), (50, w.A, w.A), (20, w.A, w.C)],
         sels=([0, 1, 2, 3],))
    return out


def draw_residual(rng, reads, ref, genome, n):
    """n residual mutations from four sources -- alleles of read entries, the reference base at covered positions,
    positions where reads have N, random -- plus repeats of a position with another allele, in both orders"""
    pos, _, mut, _ = w.unpack_read_word(reads.read_word)
    real = np.flatnonzero((mut != 15) & (pos >= 1) & (pos <= genome))
    isn = np.flatnonzero((mut == 15) & (pos >= 1) & (pos <= genome))
    base = lambda p: int(ref.get(int(p), 1))
    res = []
    for _ in range(n):
        src = int(rng.integers(0, 4))
        if src == 0 and real.size:
            j = int(rng.choice(real))
            res.append((int(pos[j]), base(pos[j]), int(mut[j])))
        elif src == 1 and reads.n_reads:
            r = int(rng.integers(0, reads.n_reads))
            p = int(rng.integers(int(reads.start[r]), min(int(reads.end[r]), genome) + 1)) if reads.start[r] <= genome else genome
            res.append((p, base(p), base(p)))
        elif src == 2 and isn.size:
            j = int(rng.choice(isn))
            res.append((int(pos[j]), base(pos[j]), int(rng.integers(1, 15))))
        else:
            p = int(rng.integers(1, genome + 1))
            res.append((p, base(p), int(rng.integers(1, 15))))
        if rng.random() < 0.3:
            # the position again with another allele, after or before its first mention
            p, rf, mu = res[-1]
            other = rf if (mu != rf and rng.random() < 0.5) else int(rng.choice([a for a in range(1, 15) if a != mu]))
            if rng.random() < 0.5:
                res.append((p, rf, other))
            else:
                res.insert(int(rng.integers(0, len(res))), (p, rf, other))
    return res


def repeated_positions(residual):
    """positions listed more than once with different alleles, and the number of such pairs whose first / second
    member is the reference allele (the two orders of a pair the three-way rule tells apart)"""
    seen = {}
    ref_first = ref_second = 0
    for p, rf, mu in residual:
        for earlier in seen.get(p, []):
            if earlier != mu:
                ref_first += earlier == rf
                ref_second += mu == rf
        seen.setdefault(p, []).append(mu)
    return [p for p, v in seen.items() if len(set(v)) > 1], ref_first, ref_second


def long_list_case(n_reads):
    """one relation list of n_reads reads: identical windows under a reference-allele mutation; every third read
    carries A5C, so the reads' nearest haplotypes differ; a second mutation nobody meets"""
    tree, ref = hand_tree()
    reads = [[(5, w.A, w.C)] if i % 3 == 0 else [] for i in range(n_reads)]
    degree = [1 + i % 5 for i in range(n_reads)]
    rd = w.EppReads.from_lists(reads, [3] * n_reads, [30] * n_reads, degree)
    return tree, rd, GENOME, np.array([0, 1, 2, 3], np.uint32), [(55, w.A, w.T), (20, w.A, w.A)]


def reference_of(gen_tree, reads):
    """position -> one-hot reference base of a generated tree, as far as its mutations and the reads tell (A elsewhere:
    wepp_epp_resolve compares ref_nuc with mut_nuc only)"""
    ref = {}
    t = gen_tree.tree
    for p, r in zip(t.mut_pos.tolist(), t.mut_ref.tolist()):
        if p > 0 and r and not (r & (r - 1)):
            ref[p] = r
    pos, rf, _, _ = w.unpack_read_word(reads.read_word)
    for p, r in zip(pos.tolist(), rf.tolist()):
        if r and not (r & (r - 1)):
            ref[p] = r
    return ref
