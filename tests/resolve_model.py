"""A literal, sequential restatement of arena::resolve_unaccounted_mutations (src/WEPP/arena.cpp:746-892) as the
model of wepp_epp_resolve: per read the residual mutations inside its window in the caller's order, the entry
of the read found by a scan, an inserted N appended and the list sorted again; then per mutation its covered and
masked reads, their nearest selected haplotypes (distances from assign_model.SelectionTable, or any other
formulation handed in) and the argmax of the summed degrees over the haplotypes that appeared."""
import numpy as np

import assign_model
import wepp_amd as w

MASKED = 1 << 31
BRANCHES = ("entry_match", "entry_other", "entry_n", "absent_ref", "absent_other")


def as_triples(residual):
    if isinstance(residual, np.ndarray):
        p, r, m, _ = w.unpack_read_word(residual)
        return list(zip(p.tolist(), r.tolist(), m.tolist()))
    return [(int(p), int(r), int(m)) for p, r, m in residual]


def mask_reads(reads, residual):
    """:746-809.  Returns the modified reads (every read, the untouched ones as they were) as an EppReads,
    covered[m] / masked[m] (read indices, ascending) and a counter per branch of the three-way rule."""
    res = as_triples(residual)
    M = len(res)
    covered = [[] for _ in range(M)]
    masked = [[] for _ in range(M)]
    count = dict.fromkeys(BRANCHES, 0)
    pos, ref, mut, miss = w.unpack_read_word(reads.read_word)
    new_reads = []
    for i in range(reads.n_reads):
        a, b = int(reads.read_off[i]), int(reads.read_off[i + 1])
        start, end = int(reads.start[i]), int(reads.end[i])
        rp = [[int(pos[j]), int(ref[j]), int(mut[j]), int(miss[j])] for j in range(a, b)]
        for m, (p, rf, mu) in enumerate(res):                   # copy_if :752-755 keeps the caller's order
            if not (p >= start and p <= end):
                continue
            site_found = False
            for e in rp:                                        # :762-779
                if e[0] == p:
                    if e[2] != 0b1111:
                        if e[2] == mu:
                            e[2] = 0b1111
                            e[3] = 1
                            covered[m].append(i)
                            count["entry_match"] += 1
                        else:
                            count["entry_other"] += 1
                    else:
                        masked[m].append(i)
                        count["entry_n"] += 1
                    site_found = True
                    break
            if not site_found:
                if mu == rf:                                    # :780-790
                    rp.append([p, rf, 0b1111, 1])
                    rp.sort()
                    covered[m].append(i)
                    count["absent_ref"] += 1
                else:
                    count["absent_other"] += 1
        new_reads.append([tuple(e) for e in rp])
    modified = w.EppReads.from_lists(new_reads, reads.start, reads.end, reads.degree)
    return modified, covered, masked, count


def tally(modified, covered, masked, K, dist_of_read):
    """:833-892 with d(r', .) = dist_of_read(r): an int array over the K selected haplotypes"""
    M = len(covered)
    KW = (K + 31) // 32
    hap_reads = np.zeros((M, K), np.uint32)
    hap_degree = np.zeros((M, K), np.int64)
    best_degree = np.zeros(M, np.int64)
    best_mask = np.zeros((M, KW), np.uint32)
    best, rel = [], []
    rel_off = np.zeros(M + 1, np.uint64)
    touched = set()
    epps = {}
    for m in range(M):
        pairs = sorted([(r, 0) for r in covered[m]] + [(r, MASKED) for r in masked[m]])
        rel += [r | f for r, f in pairs]
        rel_off[m + 1] = rel_off[m] + np.uint64(len(pairs))
        count = {}                                              # hap_reads_count: only haplotypes that appeared
        for r, _ in pairs:
            touched.add(r)
            if r not in epps:
                d = np.asarray(dist_of_read(r))
                epps[r] = np.flatnonzero(d == d.min())
            for k in epps[r].tolist():
                count[k] = count.get(k, 0) + int(modified.degree[r])
                hap_reads[m, k] += 1
        for k, v in count.items():
            hap_degree[m, k] = v
        mx = max(count.values()) if count else 0
        bk = sorted(k for k, v in count.items() if v == mx)
        best_degree[m] = mx
        best.append(np.array(bk, np.uint32))
        for k in bk:
            best_mask[m, k // 32] |= np.uint32(1 << (k & 31))
    return dict(rel_off=rel_off, rel_read=np.array(rel, np.uint32),
                n_covered=np.array([len(c) for c in covered], np.uint32),
                n_masked=np.array([len(c) for c in masked], np.uint32), best_degree=best_degree, best_mask=best_mask,
                best=best, hap_reads=hap_reads, hap_degree=hap_degree, n_touched=len(touched))


def resolve(tree, reads, genome_size, sel, residual, flat=None, table=None):
    """What Mat.epp_resolve returns (with lists and tallies), plus `modified` (the reads r') and `branches`."""
    tab = table if table is not None else assign_model.SelectionTable(tree, sel, flat)
    modified, covered, masked, count = mask_reads(reads, residual)
    pos, _, mut, _ = w.unpack_read_word(modified.read_word)

    def dist(r):
        a, b = int(modified.read_off[r]), int(modified.read_off[r + 1])
        return tab.distances(pos[a:b], mut[a:b], int(modified.start[r]), int(modified.end[r]))
    out = tally(modified, covered, masked, tab.sel.size, dist)
    out["modified"] = modified
    out["branches"] = count
    return out


KEYS = ("rel_off", "rel_read", "n_covered", "n_masked", "best_degree", "best_mask", "hap_reads", "hap_degree")


def check_equal(got, want, tag=""):
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (tag, k)
    assert int(got["n_touched"]) == int(want["n_touched"]), (tag, "n_touched")
    assert len(got["best"]) == len(want["best"]), (tag, "best")
    for m, (a, b) in enumerate(zip(got["best"], want["best"])):
        assert np.array_equal(a, b), (tag, "best", m)
