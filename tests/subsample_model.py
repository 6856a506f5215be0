r"""Model of read subsampling (wepp_sam_build_subsampled; the reference's sam::subsample, src/WEPP/sam2pb.cpp:362-454)
on top of sam_model.py, in plain Python / numpy.

The draw is the library's, not the reference's std::shuffle of a random_device-seeded mt19937:
  f(x)        the splitmix64 finaliser on 64-bit unsigned integers
  h_t         = f(seed ^ f(t))
  key(t, r)   = f(h_t ^ r)          (f is a bijection: the keys of one trial are distinct)
  subset of t = the m reads with the smallest keys = {r : key(t, r) <= thr_t}, thr_t the m-th smallest key
The full table F is sam_model.frequency_table (N not counted, '_' counted); the trial table A_t piles up the subset
with N counted too (:419-426).  With S_i / A_i the six columns' sums of site i, C / C_t the sites with S_i / A_i > 0:
  p_ij = F_ij / (S_i * C)     q_ij = A_ij / (A_i * C_t), 0 when A_i = 0
  D_t  = sum over the cells with F_ij > 0, in site order, of p_ij * (ln p_ij - ln max(q_ij, 1e-10))
every operation an IEEE double operation in the order written (the products S_i * C are exact); the sum through
math.fsum.  The winner is the trial of the smallest D_t, the lowest t among equals.  The kept reads are corrected with
the keep table of the FULL table (:394, :281-314), then sorted and merged as sam_model.build does it.

bound_t = 4 * (terms + 8) * 2^-52 * sum |term| bounds what a device sum of the same terms may differ by: fp64
summation of `terms` addends in any order stays within (terms - 1) * 2^-53 * sum |term| to first order, and a
logarithm that is off by one ulp moves a term by about 2^-52 of its factors; the factor 4 and the 8 are head-room."""
import math

import numpy as np

import sam_model as sm

MASK = (1 << 64) - 1
Q_FLOOR = 1e-10


def f(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def trial_hash(seed, t):
    return f((seed & MASK) ^ f(t))


def key(seed, t, r):
    return f(trial_hash(seed, t) ^ r)


def _f_np(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def keys(seed, t, n):
    """key(t, r) for r = 0 .. n - 1 as uint64 (the same function as key(), vectorised)"""
    return _f_np(np.uint64(trial_hash(seed, t)) ^ np.arange(n, dtype=np.uint64))


def threshold(seed, t, n, m):
    """thr_t: the m-th smallest key of trial t (1 <= m <= n)"""
    return int(np.partition(keys(seed, t, n), m - 1)[m - 1])


def subset(seed, t, n, m):
    """ascending input indices of the m reads of trial t"""
    k = keys(seed, t, n)
    return np.flatnonzero(k <= np.uint64(threshold(seed, t, n, m))).tolist()


def _cells(reads):
    """per aligned column: (read, cell = site * 6 + code)"""
    owner = np.repeat(np.arange(len(reads)), [len(r[2]) for r in reads])
    code = np.frombuffer("".join(r[2] for r in reads).translate(str.maketrans("ACGTN_", "\0\1\2\3\4\5")).encode("latin1"), np.uint8)
    site = np.concatenate([np.arange(r[1], r[1] + len(r[2])) for r in reads]) if reads else np.zeros(0, np.int64)
    return owner, site.astype(np.int64) * 6 + code, code


def trial_table(reads, genome_size, members, cells=None):
    """A_t: the pile-up of the reads `members` (a boolean vector per read), N counted"""
    owner, cell, _ = cells or _cells(reads)
    return np.bincount(cell[members[owner]], minlength=genome_size * 6).reshape(genome_size, 6)


def divergence(F, A):
    """(D_t, bound_t) of the full table F and a trial table A (integer arrays [G][6])"""
    S, At = F.sum(axis=1), A.sum(axis=1)
    C, Ct = int((S > 0).sum()), int((At > 0).sum())
    terms = []
    for i in np.flatnonzero(S > 0).tolist():
        for j in range(6):
            if F[i, j] == 0:
                continue
            p = float(F[i, j]) / (float(S[i]) * float(C))
            q = float(A[i, j]) / (float(At[i]) * float(Ct)) if At[i] > 0 else 0.0
            terms.append(p * (math.log(p) - math.log(max(q, Q_FLOOR))))
    return math.fsum(terms), 4.0 * (len(terms) + 8) * 2.0 ** -52 * math.fsum(abs(x) for x in terms)


def build_kept(reference, reads, kept, freq, min_af, min_depth):
    """sam_model.build for the reads `kept` (ascending input indices) under the keep table of `freq`; order names
    input reads"""
    sub = [reads[i] for i in kept]
    corrected = sm.correct(sub, freq, min_af, min_depth)
    order = sorted(range(len(sub)), key=lambda i: (corrected[i][1], len(corrected[i][2]), corrected[i][2], i))
    group_off = []
    for s, i in enumerate(order):
        if s == 0 or (corrected[i][1], corrected[i][2]) != (corrected[order[s - 1]][1], corrected[order[s - 1]][2]):
            group_off.append(s)
    group_off.append(len(order))
    m = dict(freq=freq, corrected=corrected, order=[kept[i] for i in order], group_off=group_off, start=[], end=[], degree=[],
             name=[], content=[], read_off=[0], read_word=[], reverse_columns={})
    for g in range(len(group_off) - 1):
        lo, hi = group_off[g], group_off[g + 1]
        name, start, s = corrected[order[lo]]
        degree = hi - lo
        m["start"].append(start + 1)
        m["end"].append(start + len(s))
        m["degree"].append(degree)
        gen = sm.degree_name(name, start, len(s), degree)
        m["name"].append(gen)
        m["content"].append(s)
        m["reverse_columns"].setdefault(gen, []).extend(corrected[order[k]][0] for k in range(lo, hi))
        for j, ch in enumerate(s):
            ref_c = reference[start + j]
            if ch != ref_c and ch != "_":
                m["read_word"].append(sm.pack_word(start + 1 + j, sm.nuc_id(ref_c), sm.nuc_id(ch), ch == "N"))
        m["read_off"].append(len(m["read_word"]))
    return m


def subsample(reference, reads, min_af, min_depth, seed, max_reads, trials):
    """The whole call.  Returns sam_model.build's dict for the kept reads (freq = the FULL table) plus kept, best_trial
    (None when nothing was drawn), threshold[T], divergence[T], bound[T], tables (the trials' tables, for the tests'
    own conditions)."""
    n, G = len(reads), len(reference)
    if n <= max_reads:
        m = sm.build(reference, reads, min_af, min_depth)
        m.update(kept=list(range(n)), best_trial=None, threshold=[0] * trials, divergence=[0.0] * trials, bound=[0.0] * trials, tables=[])
        return m
    F = np.array(sm.frequency_table(reads, G), np.int64).reshape(G, 6)
    cells = _cells(reads)
    thr, div, bound, tables = [], [], [], []
    for t in range(trials):
        k = keys(seed, t, n)
        thr.append(int(np.partition(k, max_reads - 1)[max_reads - 1]))
        A = trial_table(reads, G, k <= np.uint64(thr[-1]), cells)
        d, b = divergence(F, A)
        div.append(d); bound.append(b); tables.append(A)
    best = min(range(trials), key=lambda t: (div[t], t))
    kept = np.flatnonzero(keys(seed, best, n) <= np.uint64(thr[best])).tolist()
    m = build_kept(reference, reads, kept, F.tolist(), min_af, min_depth)
    m.update(kept=kept, best_trial=best, threshold=thr, divergence=div, bound=bound, tables=tables)
    return m


def separated(m):
    """The condition a GPU case must meet: every trial whose table differs from the winner's exceeds the winner's
    divergence by more than the sum of the two bounds.  Returns the smallest (gap - bounds) over those trials, or
    None when every table equals the winner's."""
    b = m["best_trial"]
    worst = None
    for t, A in enumerate(m["tables"]):
        if np.array_equal(A, m["tables"][b]):
            continue
        slack = m["divergence"][t] - m["divergence"][b] - (m["bound"][t] + m["bound"][b])
        worst = slack if worst is None else min(worst, slack)
    return worst
