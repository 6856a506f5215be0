"""The two forms of the peak loop's model (tests/peaks_model.py) agree: the line-by-line restatement of
wepp_filter::step and what it calls (with its EPP cache at three sizes, so that the cached and the recomputing branch
both run) equals the closed form wepp_epp_peaks computes -- on everything except the scores of mapped haplotypes, which
the reference leaves dependent on the cache.  That equality is what the device design rests on."""
import pytest

import peaks_model as pm

MAX_CACHED = (0, 3, 2048)


@pytest.fixture(scope="module")
def fuzz():
    """(index, parameters) -> closed result, or None where the model refuses a near tie; computed once"""
    problems, closed = {}, {}
    for it, pb in pm.fuzz_problems():
        problems[it] = pb
        for par in pm.PARAMS:
            try:
                closed[it, par] = pm.peaks_closed(pb, *par)
            except pm.Ambiguous:
                closed[it, par] = None
    return problems, closed


def test_literal_equals_closed_on_the_fuzz_set(fuzz):
    problems, closed = fuzz
    ran = 0
    for (it, par), want in closed.items():
        if want is None:
            continue
        for mc in MAX_CACHED:
            pm.check_equal(pm.peaks_literal(problems[it], *par, max_cached=mc), want, (it, par, mc))
        ran += 1
    assert ran >= 100


def test_near_ties_are_rare_and_the_set_is_not_vacuous(fuzz):
    _, closed = fuzz
    refused = sum(1 for v in closed.values() if v is None)
    assert refused * 10 <= len(closed), "more than 10 % of the fuzz cases are near ties: choose other seeds"
    busy = sum(1 for v in closed.values() if v is not None and v["n_steps"] > 1 and v["rejected"] > 0)
    assert busy * 3 >= len(closed), "fewer than a third of the runs take more than one step and reject a candidate"


def test_the_cache_decides_the_scores_of_mapped_haplotypes_only(fuzz):
    """the recomputing branch leaves mapped haplotypes out of a removal: somewhere on the set the two cache sizes differ
    in a mapped haplotype's score -- and nowhere in an unmapped one's (check_equal above)"""
    problems, closed = fuzz
    differs = 0
    for (it, par), want in closed.items():
        if want is None or differs:
            continue
        a = pm.peaks_literal(problems[it], *par, max_cached=0)
        differs += any(a["score"][h] != want["score"][h] for h in range(problems[it].N) if want["mapped"][h])
    assert differs


@pytest.mark.parametrize("name", sorted(pm.hand_cases()))
def test_hand_cases(name):
    tree, reads, par, exp = pm.hand_cases()[name]
    pb = pm.Problem(tree, reads, pm.GENOME)
    want = pm.peaks_closed(pb, *par)                         # (Ambiguous here fails the test: none of these is a near tie)
    pm.check_expectations(want, exp, name)
    for mc in MAX_CACHED:
        pm.check_equal(pm.peaks_literal(pb, *par, max_cached=mc), want, (name, mc))


def test_tie_rank_orders_a_group():
    tree, reads, _, _ = pm.hand_cases()["star_12_top_n_10"]
    pb = pm.Problem(tree, reads, pm.GENOME)
    rank = [0] + list(range(12, 0, -1))                      # the leaves in reverse
    want = pm.peaks_closed(pb, 10, 300, 0, tie_rank=rank)
    assert [int(x) for x in want["peaks"]] == list(range(12, 0, -1))
    pm.check_equal(pm.peaks_literal(pb, 10, 300, 0, tie_rank=rank), want, "ranks")
