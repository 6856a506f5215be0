"""wepp_sam_build on the GPU against the line-by-line model (tests/sam_model.py), bit for bit in every output: the
frequency table, the order, the groups, and the merged batch's starts, ends, degrees and word CSR.  Every test first
asserts that the MODEL's answer shows the edge it is about, so a change of a generator cannot hollow it out.

Layout units whose two sides are covered (sam.hpp, sam_kernels.hip): 256 places per workgroup of k_sam_heads and
k_sam_groups (groups straddle places 256, 512 and 768, and one ends at the last read); a wave of 64 read windows and a
workgroup round of 256 in k_sam_pileup; 64 columns per wave round of k_sam_words (reads of 1 .. 40 columns, and one of
2100); 4 merged reads per workgroup of k_sam_merge; the pile-up tile of 2048 sites (a read that crosses it); LDS
counters that take more than 256 and more than 65 536 columns of one site before they are flushed."""
import random

import numpy as np
import pytest

import sam_model as sm
import wepp_amd as w

pytestmark = pytest.mark.gpu

def encode(reads):
    start = np.array([r[1] for r in reads], np.uint32)
    base_off = np.zeros(len(reads) + 1, np.uint64)
    base_off[1:] = np.cumsum([len(r[2]) for r in reads])
    base = np.frombuffer("".join(r[2] for r in reads).translate(str.maketrans("ACGTN_", "\0\1\2\3\4\5")).encode("latin1"), np.uint8)
    return start, base_off, base


def check(got, m, tag=""):
    assert np.array_equal(got["freq"], np.array(m["freq"], np.int32).reshape(-1, 6)), (tag, "freq")
    assert got["order"].tolist() == m["order"], (tag, "order")
    assert got["n_merged"] == len(m["start"]), (tag, "n_merged")
    assert got["group_off"].tolist() == m["group_off"], (tag, "group_off")
    rd = got["reads"]
    assert rd.start.tolist() == m["start"] and rd.end.tolist() == m["end"], (tag, "windows")
    assert rd.degree.tolist() == m["degree"], (tag, "degree")
    assert rd.read_off.tolist() == m["read_off"], (tag, "read_off")
    assert rd.read_word.tolist() == m["read_word"], (tag, "read_word")


def run(ref, reads, min_af, min_depth, **kw):
    m = sm.build(ref, reads, min_af, min_depth)
    got = w.sam_build(ref, *encode(reads), min_af=min_af, min_depth=min_depth, **kw)
    return got, m


AF = sm.stof("0.005")


@pytest.mark.parametrize("part", range(4))
def test_fuzz(part):
    """32 seeds: reads of 1 .. 40 columns on genomes of 64 .. 300 sites, a handful of templates with sparse changes"""
    for seed in range(part, 32, 4):
        ref, reads = sm.gen_aligned(1000 + seed)
        rng = random.Random(seed)
        min_af, min_depth = rng.choice([AF, 0.02, 0.0]), rng.choice([0, 3, 10])
        got, m = run(ref, reads, min_af, min_depth)
        assert 64 <= len(ref) <= 300 and all(1 <= len(r[2]) <= 40 for r in reads)
        assert len(m["start"]) < len(reads) and max(m["degree"]) > 1 and m["read_word"], "no duplicates or no words in the model"
        assert any(a[2] != b[2] for a, b in zip(reads, m["corrected"])), "the correction changed nothing"
        check(got, m, seed)


def test_group_sizes():
    """groups of 1, 2, 63, 64, 65, 255, 256 and 257 equal reads, their members spread over the file; in the sorted
    order the group of 2 straddles place 256, the group of 256 place 512, the group of 257 place 768 and ends at the
    last read"""
    rng = random.Random(5)
    ref = sm.random_reference(rng, 128)
    sizes = [255, 2, 63, 64, 65, 1, 256, 257]
    reads = []
    for k, n in enumerate(sizes):
        s = ref[k:k + 20]
        s = s[:3] + ("N" if s[3] != "N" else "A") + s[4:]
        reads += [(None, k, s)] * n
    rng.shuffle(reads)
    reads = [(f"r{i}", st, s) for i, (_, st, s) in enumerate(reads)]
    got, m = run(ref, reads, 0.0, 0)
    assert m["degree"] == sizes
    for b in (256, 512, 768):
        assert any(m["group_off"][g] < b < m["group_off"][g + 1] for g in range(len(sizes))), b
    assert m["group_off"][-1] == len(reads) and m["degree"][-1] == 257
    # the earliest member in the file leads, the members follow in file order
    for g in range(len(sizes)):
        members = m["order"][m["group_off"][g]:m["group_off"][g + 1]]
        assert members == sorted(members)
    check(got, m)


def test_one_group_holds_every_read():
    rng = random.Random(6)
    ref = sm.random_reference(rng, 64)
    reads = [(f"r{i}", 7, ref[7:30]) for i in range(600)]
    got, m = run(ref, reads, AF, 10)
    assert m["degree"] == [600] and m["read_word"] == []
    check(got, m)


REF16 = "ACGTACGTTTGCAACG"


def _ordering_cases():
    ref = REF16
    c = {}
    # equal start, different lengths: the shorter first, although it comes later in the file
    c["lengths"] = ([("a", 2, ref[2:9]), ("b", 2, ref[2:6])], [1, 0])
    # equal (start, length), different only in the first / in the last column
    c["first_column"] = ([("a", 4, "T" + ref[5:10]), ("b", 4, "C" + ref[5:10]), ("c", 4, ref[4:10])], None)
    c["last_column"] = ([("a", 4, ref[4:9] + "G"), ("b", 4, ref[4:9] + "A"), ("c", 4, ref[4:10])], None)
    # N against T where the reference has A (two words) and where it has T (one word): N first, ASCII not column order
    c["n_before_t"] = ([("a", 0, "T" + ref[1:5]), ("b", 0, "N" + ref[1:5])], [1, 0])
    c["n_before_ref_t"] = ([("a", 3, ref[3:8]), ("b", 3, "N" + ref[4:8])], [1, 0])
    # word lists of different lengths that first differ where only one read has a word
    c["one_has_a_word"] = ([("a", 0, "ACGTAGGT"), ("b", 0, "ATGTAGGT"), ("c", 0, "AAGTAGGT")], [2, 0, 1])
    return ref, c


@pytest.mark.parametrize("name", ["lengths", "first_column", "last_column", "n_before_t", "n_before_ref_t", "one_has_a_word"])
def test_ordering(name):
    ref, cases = _ordering_cases()
    reads, want_order = cases[name]
    got, m = run(ref, reads, 0.0, 0)
    if want_order is not None:
        assert m["order"] == want_order, "the model does not show the order the case is about"
    else:
        strings = [m["corrected"][i][2] for i in m["order"]]
        assert strings == sorted(strings) and len(set(strings)) == len(strings)
    assert len(m["start"]) == len(reads)
    if name == "one_has_a_word":
        n = [m["read_off"][g + 1] - m["read_off"][g] for g in range(3)]
        assert sorted(n) == [1, 2, 2] and n[1] == 1      # places: AAGTAGGT (2 words), ACGTAGGT (1), ATGTAGGT (2)
    check(got, m, name)


def test_equal_after_correction_merge():
    """a read with a rare C and a read with N at the same column are different reads before the correction and one
    merged read after it"""
    ref = REF16
    reads = [(f"m{i}", 0, ref[0:6]) for i in range(40)] + [("c", 0, "AC" + "C" + ref[3:6]), ("n", 0, "AC" + "N" + ref[3:6])]
    got, m = run(ref, reads, 0.05, 10)
    assert reads[40][2] != reads[41][2] and m["corrected"][40][2] == m["corrected"][41][2] == "ACNTAC"
    assert m["degree"] == [40, 2] and m["order"][-2:] == [40, 41]
    check(got, m)


def _hair_pair(min_af, max_total=2000):
    """(c, total) closest to min_af - 1e-9 from below (becomes N) and from above-or-equal (kept), by the model's own test"""
    cut = min_af - sm.SCORE_EPSILON
    below = above = None
    for total in range(1000, max_total + 1):
        for c in (int(cut * total), int(cut * total) + 1):
            q = float(c) / float(total)
            is_n = min_af - q > sm.SCORE_EPSILON
            d = abs(q - cut)
            if is_n and (below is None or d < below[0]):
                below = (d, c, total)
            if not is_n and (above is None or d < above[0]):
                above = (d, c, total)
    return below[1:], above[1:]


def test_threshold():
    """cells at c / total = 1/200, 1/201, 1/199, 5/1000 and a hair on either side of min_af - 1e-9 under
    min_af = (double)stof("0.005"); total == min_depth (kept) and min_depth - 1 (all N)"""
    min_af, min_depth = AF, 10
    below, above = _hair_pair(min_af)
    cells = [(1, 200), (1, 201), (1, 199), (5, 1000), below, above]
    ref = "A" * (len(cells) + 2)
    reads = []
    for site, (c, total) in enumerate(cells):
        reads += [(f"s{site}c{i}", site, "C") for i in range(c)] + [(f"s{site}a{i}", site, "A") for i in range(total - c)]
    d_eq, d_less = len(cells), len(cells) + 1
    reads += [(f"d{i}", d_eq, "C") for i in range(min_depth)] + [(f"e{i}", d_less, "C") for i in range(min_depth - 1)]
    random.Random(7).shuffle(reads)
    got, m = run(ref, reads, min_af, min_depth)
    minor_is_n = []
    for site in range(len(cells)):
        out = {m["corrected"][i][2] for i, r in enumerate(reads) if r[1] == site and r[2] == "C"}
        assert len(out) == 1
        minor_is_n.append(out == {"N"})
    assert minor_is_n == [False, True, False, False, True, False], minor_is_n
    assert {m["corrected"][i][2] for i, r in enumerate(reads) if r[1] == d_eq} == {"C"}
    assert {m["corrected"][i][2] for i, r in enumerate(reads) if r[1] == d_less} == {"N"}
    check(got, m)


def test_no_depth_and_all_n_column():
    """min_depth == 0 and a column whose every read is N: total == 0, the quotient is NaN and nothing changes"""
    ref = REF16
    reads = [(f"r{i}", 2, "GNAC") for i in range(5)] + [("x", 3, "NA")]
    got, m = run(ref, reads, AF, 0)
    assert m["freq"][3] == [0] * 6 and all(c[2] == r[2] for c, r in zip(m["corrected"], reads))
    check(got, m)


def test_gap_is_counted_and_becomes_n():
    """'_' counts towards the depth (5 + 5 reaches min_depth = 10), turns into N and yields an N word"""
    ref = REF16
    reads = [(f"g{i}", 4, "A_G") for i in range(5)] + [(f"a{i}", 4, "ACG") for i in range(5)]
    got, m = run(ref, reads, AF, 10)
    assert m["freq"][5] == [0, 5, 0, 0, 0, 5]
    assert m["content"] == ["ACG", "ANG"] and m["read_word"] == [sm.pack_word(6, 2, 15, 1)]
    check(got, m)


def test_edges_of_the_genome_deep_sites_and_a_long_read():
    """reads at site 1 and ending at the last site; a site covered by more than 256 and one by more than 65 536
    columns; a read longer than a pile-up tile, crossing from tile 0 into tile 1"""
    rng = random.Random(8)
    G = 2348
    ref = sm.random_reference(rng, G)
    long_read = list(ref[100:2200])
    for j in rng.sample(range(len(long_read)), 30):
        long_read[j] = rng.choice("ACGTN_")
    reads = [("long", 100, "".join(long_read)), ("first", 0, ref[0:9]), ("last", G - 7, ref[G - 7:G - 1] + "N")]
    reads += [(f"d{i}", 50, ref[50] if i % 3 else "N") for i in range(300)]
    alt = "C" if ref[2100] != "C" else "G"
    reads += [(f"e{i}", 2100, alt if i % 1000 == 0 else ref[2100]) for i in range(65600)]
    got, m = run(ref, reads, AF, 10)
    assert sum(1 for r in reads if r[1] <= 50 < r[1] + len(r[2])) > 256
    assert sum(m["freq"][2100]) > 65536
    assert m["start"][0] == 1 and max(m["end"]) == G and max(e - s + 1 for s, e in zip(m["start"], m["end"])) > 2048
    check(got, m)


def test_short_word_buffer_and_fetch():
    ref, reads = sm.gen_aligned(77)
    full, m = run(ref, reads, AF, 3)
    assert len(m["read_word"]) > 4
    for cap in (0, len(m["read_word"]) - 1):
        got, _ = run(ref, reads, AF, 3, word_capacity=cap)
        check(got, m, cap)
    check(full, m)
    # nothing is pending after the fetch
    assert w._lib.lib.wepp_sam_fetch_words(None, 0) == 1


def test_no_reads():
    got = w.sam_build("ACGT" * 20, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint8), AF, 10)
    assert got["n_merged"] == 0 and got["group_off"].tolist() == [0] and not got["freq"].any() and got["reads"].n_reads == 0


@pytest.mark.parametrize("name", ["base_byte", "start", "end", "empty", "descending", "first_offset"])
def test_invalid(name):
    ref = "ACGT" * 20
    start, off, base = np.array([0, 70], np.uint32), np.array([0, 5, 12], np.uint64), np.zeros(12, np.uint8)
    want = {"base_byte": "0..5", "start": "does not lie inside", "end": "does not lie inside", "empty": "is empty",
            "descending": "does not ascend", "first_offset": "base_off[0]"}[name]
    if name == "base_byte":
        base[11] = 6
    elif name == "start":
        start[1] = 80
    elif name == "end":
        start[1] = 74
    elif name == "empty":
        off[1] = 0
    elif name == "descending":
        off[1] = 13
    else:
        off[0] = 1
    with pytest.raises(w.WeppError) as ei:
        w.sam_build(ref, start, off, base, AF, 10)
    assert ei.value.code == 1 and want in str(ei.value)
