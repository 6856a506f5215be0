"""Model of wepp_epp_peaks: the peak-removal loop of wepp_filter (src/WEPP/initial_filter.cpp:241-453) in two forms,
on top of epp_model (the map), assign_model (haplotype::mutation_distance of a read) and neighbors_model (stack_muts,
the distance between haplotypes, the regions).

  peaks_literal   follows the reference line by line: `current` kept sorted by score_comparator, remaining_reads,
                  epp_positions_cache (reads with at most max_cached placements; the others recompute their distances
                  and their EPP set WITHOUT the mapped haplotypes, single_read_tree :126-134), singular_step per accepted
                  peak in order.  Scores are fractions.Fraction.
  peaks_closed    the five steps wepp_place.h states for wepp_epp_peaks: what the device computes.

Both give the same peaks, steps, removed reads, mapped flags and scores of unmapped haplotypes (test_peaks_model.py);
the scores of mapped haplotypes depend on the reference's cache and are not compared.

Near ties.  The device sums the scores in fixed point, the reference in doubles, this model exactly.  Where a live full
score lies between 1e-12 and 1e-7 below the leader's, or the leader's lies in (1e-10, 1e-8), the three may part:
peaks_closed raises Ambiguous there and the tests skip the case."""
import functools
import math
from fractions import Fraction

import numpy as np

import assign_model as am
import epp_model
import neighbors_model as nm
import wepp_amd as w

EPS = 1e-9
NEAR_LO, NEAR_HI = 1e-12, 1e-7
M_LO, M_HI = 1e-10, 1e-8


class Ambiguous(Exception):
    pass


class Problem:
    """everything both forms start from: the map's P, M, EPP sets, q, scores and divergence; d(r, h); the arena"""

    def __init__(self, tree, reads, genome, arena=None):
        self.tree, self.reads, self.genome = tree, reads, genome
        self.arena = arena if arena is not None else nm.Arena(tree)
        N, R = tree.n_nodes, reads.n_reads
        self.N, self.R = N, R
        fv = w.FlatView(tree)
        ew, en = fv.get("epp_word").copy(), fv.get("epp_node").copy()
        tab = am.SelectionTable(tree, np.arange(N, dtype=np.uint32), fv)
        fv.close()
        m = epp_model.epp_map(ew, en, N, reads, genome, max_cached=N)
        self.P = [int(x) for x in m["max_parsimony"]]
        self.M = [int(x) for x in m["multiplicity"]]
        self.epp = [np.asarray(l, np.int64) for l in m["lists"]]
        pos, _, mut, _ = w.unpack_read_word(reads.read_word)
        self.D = np.zeros((R, N), np.int32)          # haplotype::mutation_distance(read) as wepp_epp_assign defines it
        for r in range(R):
            a, b = int(reads.read_off[r]), int(reads.read_off[r + 1])
            self.D[r] = tab.distances(pos[a:b], mut[a:b], int(reads.start[r]), int(reads.end[r]))
        self.q = [Fraction(int(reads.degree[r]), (1 + self.P[r]) * self.M[r]) for r in range(R)]
        self.score = [Fraction(0)] * N
        for r in range(R):
            for h in self.epp[r]:
                self.score[h] += self.q[r]
        # dist_divergence, initial_filter.cpp:214-233
        counts = m["counts"]
        bin_size = genome // 50
        true = np.zeros(50, np.int64)
        for r in range(R):
            true[min(int(reads.start[r]) // bin_size, 49)] += int(reads.degree[r])
        active = int((true != 0).sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            prop = counts.astype(np.float64) / true.astype(np.float64)[None, :]
            self.div = (prop > 0.5 / 100).sum(axis=1) / np.float64(active) if active else np.full(N, np.nan)

    def full(self, score, h):
        return float(score[h]) * math.sqrt(float(self.div[h]))

    def hap_dist(self, old, c):
        """old->mutation_distance(c)"""
        return self.arena.dist(nm.FROM, old, c)


def _rank_key(tie_rank, h):
    return (int(tie_rank[h]) if tie_rank is not None else 0, h)


def _result(pb, peaks, peak_step, removed_step, removed_peak, mapped, score, n_steps, rejected):
    R = pb.R
    peak_reads = [sum(1 for r in range(R) if removed_peak[r] == k) for k in range(len(peaks))]
    peak_degree = [sum(int(pb.reads.degree[r]) for r in range(R) if removed_peak[r] == k) for k in range(len(peaks))]
    return dict(peaks=np.array(peaks, np.uint32), peak_step=np.array(peak_step, np.uint32), peak_reads=np.array(peak_reads, np.uint32),
                peak_degree=np.array(peak_degree, np.int64), n_steps=n_steps, n_remaining=sum(1 for s in removed_step if s < 0),
                removed_step=np.array(removed_step, np.int32).reshape(R),
                removed_peak=np.array([0xFFFFFFFF if p < 0 else p for p in removed_peak], np.uint32).reshape(R),
                mapped=np.array(mapped, np.uint8), score=list(score), rejected=rejected)


def peaks_closed(pb, top_n=10, max_peaks=300, peak_radius=2, eps=EPS, tie_rank=None, check_near=True):
    N, R = pb.N, pb.R
    score = list(pb.score)
    mapped = [False] * N
    remaining = set(range(R))
    peaks, peak_step, removed_step, removed_peak = [], [], [-1] * R, [-1] * R
    n_steps = rejected = 0
    while R and len(peaks) < max_peaks and remaining:
        # 1. leader
        live = [h for h in range(N) if not mapped[h] and float(score[h]) > eps]
        if not live:
            break
        fs = {h: pb.full(score, h) for h in live}
        m = max(fs.values())
        if check_near:
            if M_LO < m < M_HI:
                raise Ambiguous("leader %g" % m)
            for h in live:
                if NEAR_LO < m - fs[h] < NEAR_HI:
                    raise Ambiguous("full score %g below the leader" % (m - fs[h]))
        if m < eps:
            break
        group = sorted((h for h in live if m - fs[h] < eps), key=lambda h: _rank_key(tie_rank, h))
        # 2. consideration
        acc = []
        for c in group:
            if not (len(acc) < top_n and len(acc) + len(peaks) < max_peaks):
                break
            if all(pb.hap_dist(old, c) > peak_radius for old in acc):
                acc.append(c)
            else:
                rejected += 1
        base = len(peaks)
        for c in acc:
            mapped[c] = True
            peaks.append(c); peak_step.append(n_steps)
        # 3. clear
        for a in acc:
            for node in pb.arena.possible_neighbors(a, peak_radius):
                mapped[node] = True
        # 4. remove
        for r in sorted(remaining):
            for k, a in enumerate(acc):
                if int(pb.D[r, a]) == pb.P[r]:
                    removed_step[r], removed_peak[r] = n_steps, base + k
                    remaining.discard(r)
                    for h in pb.epp[r]:
                        score[h] -= pb.q[r]
                    break
        n_steps += 1
    return _result(pb, peaks, peak_step, removed_step, removed_peak, mapped, score, n_steps, rejected)


def peaks_literal(pb, top_n=10, max_peaks=300, peak_radius=2, eps=EPS, tie_rank=None, max_cached=2048):
    N, R = pb.N, pb.R
    score = list(pb.score)
    mapped = [False] * N
    if R == 0:
        return _result(pb, [], [], [], [], mapped, score, 0, 0)
    # wepp_filter::cartesian_map :189-196
    cache = [sorted(int(h) for h in pb.epp[r]) if pb.M[r] <= max_cached else [] for r in range(R)]
    remaining_reads = set(range(R))
    full = lambda h: pb.full(score, h)

    def score_comparator(a, b):                      # arena.hpp:16-31, as a three-way comparison
        fa, fb = full(a), full(b)
        if abs(fa - fb) > eps:
            return -1 if fa > fb else 1
        ka, kb = _rank_key(tie_rank, a), _rank_key(tie_rank, b)
        return -1 if ka < kb else (1 if ka > kb else 0)
    key = functools.cmp_to_key(score_comparator)
    current = sorted(range(N), key=key)
    peaks, peak_step, removed_step, removed_peak = [], [], [-1] * R, [-1] * R
    state = dict(n_steps=0, rejected=0)

    def find_correspondents(hap):
        out = []
        for read in sorted(remaining_reads):
            c = cache[read]
            if hap in c:
                out.append(read)
            elif len(c) == pb.M[read]:
                continue
            elif int(pb.D[read, hap]) == pb.P[read]:
                out.append(read)
        return out

    def remove_read(read):
        if len(cache[read]) == pb.M[read]:
            epps = cache[read]
        else:
            epps = [int(h) for h in pb.epp[read] if not mapped[h]]      # single_read_tree :126-134
        if not epps:
            return
        for h in epps:
            score[h] -= pb.q[read]                   # (the ORIGINAL multiplicity, :309-310)

    def singular_step(hap, k):
        corr = find_correspondents(hap)
        for read in corr:
            remove_read(read)
        for read in corr:
            remaining_reads.discard(read)
            removed_step[read], removed_peak[read] = state["n_steps"], k

    def step():
        consideration = []
        min_score = full(current[0])
        if min_score < eps:
            return True
        i = 0
        while (i < len(current) and abs(full(current[i]) - min_score) < eps and len(consideration) < top_n
               and len(consideration) + len(peaks) < max_peaks):
            it = current[i]
            valid = True
            for old in consideration:
                if not pb.hap_dist(old, it) > peak_radius:
                    valid = False
            if valid:
                consideration.append(it)
                mapped[it] = True
            else:
                state["rejected"] += 1
            i += 1
        base = len(peaks)
        # clear_neighbors
        for it in consideration:
            peaks.append(it); peak_step.append(state["n_steps"])
        for pivot in consideration:
            for node in pb.arena.possible_neighbors(pivot, peak_radius):
                mapped[node] = True
        for k, node in enumerate(consideration):
            singular_step(node, base + k)
        current[:] = [h for h in current if not (mapped[h] or float(score[h]) <= eps)]
        current.sort(key=key)
        state["n_steps"] += 1
        return len(peaks) >= max_peaks or not remaining_reads or not current

    while not step():
        pass
    return _result(pb, peaks, peak_step, removed_step, removed_peak, mapped, score, state["n_steps"], state["rejected"])


def check_equal(got, want, tag="", scores=True):
    """two model results: everything but the scores of mapped haplotypes"""
    for k in ("peaks", "peak_step", "peak_reads", "peak_degree", "removed_step", "removed_peak", "mapped"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    assert got["n_steps"] == want["n_steps"] and got["n_remaining"] == want["n_remaining"], (tag, "counts")
    if scores:
        for h in range(len(want["mapped"])):
            if not want["mapped"][h]:
                assert got["score"][h] == want["score"][h], (tag, "score", h)


def score_bound(pb):
    """the fixed-point bound wepp_place.h documents for hap_score, per haplotype: (reads mapped to the haplotype) *
    2^-(42 - log2(sum of degrees)); a removal is one more rounding-free integer, so the bound of the map holds"""
    total = max(int(np.asarray(pb.reads.degree, np.int64).sum()), 1)
    per = 2.0 ** -(42 - math.log2(total))
    n = np.zeros(pb.N, np.int64)
    for r in range(pb.R):
        n[pb.epp[r]] += 1
    return n * per


# ---- cases --------------------------------------------------------------------------------------------------------
PARAMS = ((10, 300, 2), (1, 300, 0), (3, 4, 1))
GENOME = 60
FUZZ_READ_SEED = 4242


def full_ref(arena, genome=GENOME):
    """a reference base for every position: the tree's where a mutation names it, A elsewhere"""
    return {p: arena.ref.get(p, w.A) for p in range(0, genome + 2)}


def fuzz_problems(n_trees=nm.FUZZ_TREES):
    """(index, Problem) over the small trees of neighbors_model.fuzz_cases() with 50-600 generated reads"""
    import epp_fuzz
    rng = np.random.default_rng(FUZZ_READ_SEED)
    for it, (tree, ar, _) in enumerate(nm.fuzz_cases(n_trees)):
        n_reads = int(rng.integers(50, 601))
        reads = epp_fuzz.random_epp_reads(rng, tree, full_ref(ar), GENOME, n_reads=n_reads)
        yield it, Problem(tree, reads, GENOME, ar)


def _reads(items):
    """[(entries, start, end, degree)] -> EppReads"""
    return w.EppReads.from_lists([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items])


def hand_cases():
    """name -> (tree, reads, params, expectations): trees of under 20 nodes whose outcome is known by hand.  Genome 60;
    arena indices = the order of the lists (every child follows its parent, siblings in order)."""
    A, C, G, T, N = w.A, w.C, w.G, w.T, w.N
    cases = {}
    # leaves 1 and 2 differ from the root at 10 and 11: distance 2 from each other
    t2 = w.Tree.from_lists([-1, 0, 0], [[], [(10, A, A, C)], [(11, A, A, C)]])
    r_tie = _reads([([(10, A, C)], 10, 10, 2), ([(11, A, C)], 11, 11, 2)])
    cases["two_tying_leaves_within_radius"] = (t2, r_tie, (10, 300, 2), dict(peaks=[1], mapped=[1, 1, 1], n_steps=1))
    cases["two_tying_leaves_beyond_radius"] = (t2, r_tie, (10, 300, 1), dict(peaks=[1, 2], n_steps=1, n_remaining=0))
    # a star with 12 leaves, each with a read of its own
    star = w.Tree.from_lists([-1] + [0] * 12, [[]] + [[(3 * i + 2, A, A, C)] for i in range(12)])
    r_star = _reads([([(3 * i + 2, A, C)], 3 * i + 2, 3 * i + 2, 1) for i in range(12)])
    cases["star_12_top_n_10"] = (star, r_star, (10, 300, 0), dict(peaks=list(range(1, 13)), n_steps=2, peak_step=[0] * 10 + [1] * 2))
    cases["max_peaks_inside_a_tie_group"] = (star, r_star, (10, 3, 0), dict(peaks=[1, 2, 3], n_steps=1, n_remaining=9))
    # a read without entries in a window no mutation touches: its EPP set is every haplotype
    r_all = _reads([([], 50, 55, 3), ([(2, A, C)], 2, 2, 5)])
    cases["read_on_every_haplotype"] = (star, r_all, (1, 300, 0), dict(first_peak=1, first_reads=2))
    # 1 mutates 7 and 8, its child 2 takes both back and mutates 30: 2 is within radius 1 of the root, but 1 between them
    # is not, so 2 lies outside the root's connected region.  0, 2 and 3 tie in step 0: 0 is accepted, 2 (rejected, not
    # mapped) keeps the share of the read at 30 that only it explains, stays live and is chosen in step 1
    tb = w.Tree.from_lists([-1, 0, 1, 0], [[], [(7, A, A, C), (8, A, A, C)], [(7, A, C, A), (8, A, C, A), (30, A, A, T)], [(20, A, A, G)]])
    r_back = _reads([([], 5, 9, 3), ([(30, A, T)], 30, 30, 1), ([], 30, 30, 3)])
    cases["back_mutation_outside_the_region"] = (tb, r_back, (10, 300, 1), dict(peaks=[0, 2], peak_step=[0, 1], mapped=[1, 0, 1, 1], n_steps=2,
                                                                              n_remaining=0, rejected=2, removed_step=[0, 1, 0]))
    cases["degree_0_reads"] = (t2, _reads([([(10, A, C)], 10, 10, 0), ([(11, A, C)], 11, 11, 3), ([(11, A, C)], 11, 12, 0)]),
                               (10, 300, 0), dict(peaks=[2], n_steps=1, n_remaining=1))
    cases["all_n_reads"] = (t2, _reads([([(10, A, N), (11, A, N)], 10, 11, 2), ([(10, A, C)], 10, 10, 1)]), (10, 300, 0),
                            dict(first_peak=1))
    # max_peaks stops the loop at one peak: the read of leaf 2 is never matched
    cases["reads_that_remain"] = (t2, _reads([([(10, A, C)], 10, 10, 5), ([(11, A, C)], 11, 11, 1)]), (10, 1, 0),
                                  dict(peaks=[1], n_remaining=1, removed_step=[0, -1]))
    cases["no_reads"] = (t2, _reads([]), (10, 300, 2), dict(peaks=[], n_steps=0, n_remaining=0))
    return cases


def check_expectations(res, exp, tag=""):
    for k, v in exp.items():
        if k == "first_peak":
            assert int(res["peaks"][0]) == v, (tag, k)
        elif k == "first_reads":
            assert int(res["peak_reads"][0]) == v, (tag, k)
        elif k in ("n_steps", "n_remaining", "rejected"):
            assert int(res[k]) == v, (tag, k, res[k])
        else:
            assert [int(x) for x in res[k]] == list(v), (tag, k, res[k])


def expansion(pb, peaks, sort_key, peak_radius, max_neighbors=50, limit=5000):
    """the five expansion rounds of wepp_filter::filter (initial_filter.cpp:473-504): peaks in ascending arena index, the
    region of radius peak_radius + k in the order of sort_key (score_comparator over the ORIGINAL scores), nodes that are
    peaks or neighbours of the round passed over, at most max_neighbors per peak; the round closest to `limit` is kept.
    Returns (neighbours ascending, round kept)."""
    nbrs, kept = set(), -1
    for k in range(5):
        curr = set()
        for pivot in sorted(int(p) for p in peaks):
            i = 0
            for node in sorted(pb.arena.possible_neighbors(pivot, peak_radius + k), key=sort_key):
                if node in peaks or node in curr:
                    continue
                curr.add(node)
                i += 1
                if i == max_neighbors:
                    break
        if len(peaks) and abs(limit - (len(curr) + len(peaks))) < abs(limit - (len(nbrs) + len(peaks))):
            nbrs, kept = curr, k
    return sorted(nbrs), kept
