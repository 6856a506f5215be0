"""tests/sam_model.py against hand-worked cases: every CIGAR letter with the aligned string written out, the phred
cut-off, the skipped lines, the refused inputs, and a worked correction / sort / merge."""
import pytest

import sam_model as sm


def line(cigar, seq, qual=None, pos=3, flag=0, name="q"):
    qual = "I" * len(seq) if qual is None else qual
    return f"{name}\t{flag}\tref\t{pos}\t60\t{cigar}\t*\t0\t0\t{seq}\t{qual}"


CASES = [
    # cigar, seq, qual, aligned string
    ("4M", "ACGT", None, "ACGT"),
    ("2X2B", "ACGT", None, "ACGT"),                      # every other letter walks like M
    ("2=2X", "ACGT", None, "AC"),                        # '=' is no letter of \d+[A-Za-z]: the chunk is passed over, as in the reference
    ("2M1P1M", "ACGT", None, "ACGT"),                    # ... P too: it takes a base of the query
    ("2M2I2M", "ACTTGT", None, "ACGT"),                  # I consumes the query and adds nothing
    ("2M3D2M", "ACGT", None, "AC___GT"),                 # D adds gaps and consumes nothing
    ("2M2N2M", "ACTTGT", None, "ACNNGT"),                # N adds N and ADVANCES the query (the reference's walk)
    ("2H4M3H", "ACGT", None, "ACGT"),                    # H does nothing
    ("2S3M1S", "TTACGA", None, "ACG"),                   # S at both ends
    ("1M2I2D1M", "ATTC", None, "A__C"),                  # I next to D
    ("1M2D2I1M", "ATTC", None, "A__C"),
    ("4M", "acgt", None, "NNNN"),                        # lower-case bases are no bases of ACGTN
    ("5M", "ARN_T", None, "ANNNT"),                      # IUPAC and '_' become N, N stays
    ("4M", "ACGT", "5455", "ANGT"),                      # phred 20 ('5') is kept, 19 ('4') is N
    ("3m1M", "ACGT", None, "ACGT"),                      # the letter class is [A-Za-z]
    ("x2My1M", "ACG", None, "ACG"),                      # what the regex does not match is passed over
    ("0M2M", "AC", None, "AC"),
]


@pytest.mark.parametrize("cigar,seq,qual,want", CASES)
def test_cigar_by_hand(cigar, seq, qual, want):
    name, start, aligned = sm.parse_line(line(cigar, seq, qual), 1, 20)
    assert (name, start, aligned) == ("q", 2, want)


def test_skipped_lines():
    assert sm.parse_line("", 1, 20) is None
    assert sm.parse_line("   ", 1, 20) is None
    assert sm.parse_line("@SQ\tSN:ref\tLN:100", 1, 20) is None
    assert sm.parse_line(line("4M", "ACGT", flag=4), 1, 20) is None
    assert sm.parse_line(line("4M", "ACGT", flag=77), 1, 20) is None          # 77 = 64 + 8 + 4 + 1
    assert sm.parse_line(line("4M", "ACGT", flag=16), 1, 20) is not None
    text = "@HD\tVN:1\n" + line("2M", "AC", name="a") + "\n\n" + line("2M", "AC", flag=4, name="u") + "\n" + line("2M", "GT", name="b", pos=9) + "\n"
    assert sm.parse_sam(text, 10) == [("a", 2, "AC"), ("b", 8, "GT")]          # the lines behind a skipped one are read


@pytest.mark.parametrize("bad,msg", [
    ("q\t0\tref\t3\t60\t4M\t*\t0\t0\tACGT", "line 1: 10 fields"),
    (line("4M", "ACGT", "*"), "line 1: no base quality"),
    (line("4M", "ACGT", "III"), "line 1: no base quality"),
    (line("5M", "ACGT"), "line 1: the CIGAR consumes more bases"),
    (line("4M", "ACGT", pos=0), "line 1: the aligned read covers 0 .. 3"),
    (line("4M", "ACGT", pos=8), "line 1: the aligned read covers 8 .. 11"),
    (line("4S", "ACGT"), "line 1: the CIGAR yields no aligned column"),
    (line("*", "ACGT"), "line 1: the CIGAR yields no aligned column"),
    (line("4M", "ACGT", pos="x"), "line 1: POS 'x' is not a number"),
])
def test_refused(bad, msg):
    with pytest.raises(sm.SamError) as ei:
        sm.parse_sam(bad + "\n", 10)
    assert msg in str(ei.value)


def test_build_by_hand():
    """12 reads over ACGTACGT: site 3 (0-based) holds 10 T and 1 G (1/11 > 0.05: kept) and one gap; site 5 is covered 3
    times, like site 4 (below min_depth 4: N)"""
    ref = "ACGTACGT"
    reads = [(f"t{i}", 2, "GT") for i in range(9)] + [("g", 2, "GG"), ("gap", 2, "G_"), ("tail", 3, "TAC"), ("tail2", 3, "TAC"), ("tail3", 3, "TAN")]
    m = sm.build(ref, reads, 0.05, 4)
    assert m["freq"][3] == [0, 0, 1, 12, 0, 1] and m["freq"][5] == [0, 2, 0, 0, 0, 0] and m["freq"][2] == [0, 0, 11, 0, 0, 0]
    assert m["content"] == ["GG", "GN", "GT", "TNN"]          # ASCII: G < N < T; sites 4 and 5 are N for all three tails
    assert m["degree"] == [1, 1, 9, 3]
    assert m["order"] == [9, 10, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13] and m["group_off"] == [0, 1, 2, 11, 14]
    assert m["start"] == [3, 3, 3, 4] and m["end"] == [4, 4, 4, 6]
    assert m["name"] == ["g_READ_3_4_1", "gap_READ_3_4_1", "t0_READ_3_4_9", "tail_READ_4_6_3"]
    assert m["reverse_columns"]["tail_READ_4_6_3"] == ["tail", "tail2", "tail3"]
    assert m["read_off"] == [0, 1, 2, 2, 4]
    assert m["read_word"] == [sm.pack_word(4, 8, 4, 0), sm.pack_word(4, 8, 15, 1), sm.pack_word(5, 1, 15, 1), sm.pack_word(6, 2, 15, 1)]


def test_threshold_is_the_float_widened():
    af = sm.stof("0.005")
    assert af != 0.005 and abs(af - 0.005) < 1e-9
    ref = "A"
    reads = [("c", 0, "C")] + [(f"a{i}", 0, "A") for i in range(200)]       # 1 / 201
    assert sm.build(ref, reads, af, 10)["corrected"][0][2] == "N"
    assert sm.build(ref, reads[:-1], af, 10)["corrected"][0][2] == "C"       # 1 / 200: min_af - 0.005 is not > 1e-9


def test_generators_cover_what_the_tests_need():
    ref, text = sm.gen_sam(3)
    reads = sm.parse_sam(text, len(ref))
    ops = set("".join(c for c in ln.split("\t")[5] if c.isalpha()) for ln in text.split("\n") if ln and ln[0] != "@" and ln.split("\t")[5] != "*")
    assert set("MIDNSHPX") <= set("".join(ops)) and len(reads) >= 100
    assert any("_" in r[2] for r in reads) and any("N" in r[2] for r in reads)
    ref, al = sm.gen_aligned(4)
    m = sm.build(ref, al, sm.stof("0.005"), 3)
    assert len(m["start"]) < len(al) // 2
