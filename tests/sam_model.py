r"""Model of `wepp sam2PB`: a line-by-line restatement of sam::add_reads, sam::read_correction, the sort under
sam_read::operator<, sam::merge_duplicates and what load_reads_from_proto makes of the written file
(src/WEPP/sam2pb.cpp:153-360, 456-477, 489-549; sam2pb.hpp:14-48), under the reference's constants
USE_READ_CORRECTION, USE_COLUMN_MERGING, !MAP_TO_MAJORITY_INSTEAD_OF_N, SCORE_EPSILON = 1e-9.

Python strings compare by code point (= ASCII here) and Python floats are IEEE doubles, so the sort and the threshold
are the reference's own expressions.  np.float32(text) stands in for std::stof.

Where the reference has no defined result the model has the library's stated behaviour: header, empty and unmapped
lines are skipped (the reference's `return` drops the rest of a TBB range); among equal reads the earliest in the file
leads; inputs on which the reference indexes out of bounds raise SamError naming the line; a '_' in SEQ becomes N
(the reference's find in "ACGTN_" would keep it).  As in the reference, a CIGAR chunk whose operator is no letter
('=') does not match \d+[A-Za-z] and is passed over.

Also holds the generators of small SAM texts and aligned-read sets the tests share."""
import random
import re

import numpy as np

GENOME_STRING = "ACGTN_"
SCORE_EPSILON = 1e-9
NUC_ID = {"A": 1, "a": 1, "C": 2, "c": 2, "G": 4, "g": 4, "T": 8, "t": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12,
          "M": 3, "B": 14, "D": 13, "H": 11}          # MAT::get_nuc_id; everything else 15


class SamError(Exception):
    pass


def stof(text):
    """dataset::min_af: the option's text through std::stof, widened to double"""
    return float(np.float32(text))


def _stoi(tok, what, where):
    m = re.match(r"[+-]?[0-9]+", tok)
    if not m:
        raise SamError(f"{where}: {what} '{tok}' is not a number")
    return int(m.group(0))


def cigar_chunks(cigar):
    r"""the matches of \d+[A-Za-z] (:176-189)"""
    return [(int(n), c) for n, c in re.findall(r"([0-9]+)([A-Za-z])", cigar)]


def parse_line(line, lineno, min_phred):
    """One SAM line -> (name, 0-based start, aligned string) or None for a skipped line (:157-258)."""
    where = f"line {lineno}"
    tokens = [t for t in re.split(r"[ \t\n\v\f\r]+", line) if t]
    if not tokens or tokens[0][0] == "@":
        return None
    if len(tokens) < 11:
        raise SamError(f"{where}: {len(tokens)} fields, at least 11 expected")
    if _stoi(tokens[1], "FLAG", where) & 4:
        return None
    start_idx = _stoi(tokens[3], "POS", where)
    seq, qual = tokens[9], tokens[10]
    if qual == "*" or len(qual) < len(seq):
        raise SamError(f"{where}: no base quality for every base of the query")
    seq_idx, build = 0, []
    for n, op in cigar_chunks(tokens[5]):
        if n > 10 ** 9:
            raise SamError(f"{where}: CIGAR length in '{tokens[5]}'")
        if op == "I":
            seq_idx += n
        elif op == "D":
            build.append("_" * n)
        elif op == "N":
            build.append("N" * n)
            seq_idx += n
        elif op == "H":
            pass
        elif op == "S":
            seq_idx += n
        else:
            for _ in range(n):
                if seq_idx >= len(seq):
                    raise SamError(f"{where}: the CIGAR consumes more bases than the query holds")
                q = ord(qual[seq_idx])
                q = q - 256 if q >= 128 else q           # (a signed char)
                alt = "N" if q - 33 < min_phred else seq[seq_idx]
                if alt not in "ACGTN":
                    alt = "N"
                build.append(alt)
                seq_idx += 1
    aligned = "".join(build)
    if not aligned:
        raise SamError(f"{where}: the CIGAR yields no aligned column")
    return tokens[0], start_idx - 1, aligned


def parse_sam(text, genome_size, min_phred=20):
    """Every mapped line of a SAM text: [(name, 0-based start, aligned string)], in file order."""
    reads = []
    for lineno, line in enumerate(text.split("\n"), 1):
        got = parse_line(line, lineno, min_phred)
        if got is None:
            continue
        name, start, aligned = got
        if start < 0 or start + len(aligned) > genome_size:
            raise SamError(f"line {lineno}: the aligned read covers {start + 1} .. {start + len(aligned)}, outside the reference 1 .. {genome_size}")
        reads.append(got)
    return reads


def nuc_id(ch):
    return NUC_ID.get(ch, 15)


def pack_word(position, ref_nuc, mut_nuc, is_missing):
    return (position & 0xFFFFF) | ((ref_nuc & 15) << 20) | ((mut_nuc & 15) << 24) | ((is_missing & 1) << 28)


def frequency_table(reads, genome_size):
    """:262-275"""
    freq = [[0] * 6 for _ in range(genome_size)]
    for _, start, s in reads:
        for i, ch in enumerate(s):
            if ch == "N":
                continue
            freq[start + i][GENOME_STRING.index(ch)] += 1
    return freq


def correct(reads, freq, min_af, min_depth):
    """sam::read_correction :282-314 (the reads' half)"""
    total = [sum(row) for row in freq]
    out = []
    for name, start, s in reads:
        al = list(s)
        for j in range(len(al)):
            indx = start + j
            curr = GENOME_STRING.index(al[j])
            if min_depth > total[indx]:
                al[j] = "N"
            else:
                # (double) freq / total with total == 0 is NaN in C++: the comparison is false
                if total[indx] != 0 and min_af - float(freq[indx][curr]) / float(total[indx]) > SCORE_EPSILON:
                    al[j] = "N"
            if al[j] == "_":
                al[j] = "N"
        out.append((name, start, "".join(al)))
    return out


def degree_name(name, start, length, degree):
    return f"{name}_READ_{start + 1}_{start + 1 + length - 1}_{degree}"


def build(reference, reads, min_af, min_depth):
    """Steps 2-5 for aligned reads [(name, 0-based start, string over ACGTN_)].  Returns a dict:
    freq [G][6]; corrected [(name, start, string)]; order (input index per place); group_off; per merged read start
    (1-based), end, degree, name (degree_name of the leader), content; read_off / read_word as load_reads_from_proto
    builds them; reverse_columns {degree_name: [member names]} as sam::dump_proto writes it (:122-129)."""
    G = len(reference)
    freq = frequency_table(reads, G)
    corrected = correct(reads, freq, min_af, min_depth)
    order = sorted(range(len(reads)), key=lambda i: (corrected[i][1], len(corrected[i][2]), corrected[i][2], i))
    group_off = []
    for s, i in enumerate(order):
        if s == 0 or (corrected[i][1], corrected[i][2]) != (corrected[order[s - 1]][1], corrected[order[s - 1]][2]):
            group_off.append(s)
    group_off.append(len(order))
    m = dict(freq=freq, corrected=corrected, order=order, group_off=group_off, start=[], end=[], degree=[], name=[],
             content=[], read_off=[0], read_word=[], reverse_columns={})
    if not reads:
        m["group_off"] = [0]
    for g in range(len(group_off) - 1):
        lo, hi = group_off[g], group_off[g + 1]
        name, start, s = corrected[order[lo]]
        degree = hi - lo
        m["start"].append(start + 1)
        m["end"].append(start + len(s))
        m["degree"].append(degree)
        gen = degree_name(name, start, len(s), degree)
        m["name"].append(gen)
        m["content"].append(s)
        m["reverse_columns"].setdefault(gen, []).extend(corrected[order[k]][0] for k in range(lo, hi))
        for j, ch in enumerate(s):
            ref_c = reference[start + j]
            if ch != ref_c and ch != "_":
                m["read_word"].append(pack_word(start + 1 + j, nuc_id(ref_c), nuc_id(ch), ch == "N"))
        m["read_off"].append(len(m["read_word"]))
    return m


# ---- generators ---------------------------------------------------------------------------------------------------
def random_reference(rng, G):
    return "".join(rng.choice("ACGT") for _ in range(G))


def gen_aligned(seed, G=None, n_reads=None, max_len=40, n_templates=6, p_sub=0.04, p_n=0.03, p_gap=0.02):
    """A reference and aligned reads with heavy duplication: a handful of templates (start, length) copied off the
    reference, each read a template with sparse substitutions, Ns and gaps."""
    rng = random.Random(seed)
    G = G or rng.randint(64, 300)
    n_reads = n_reads or rng.randint(50, 1500)
    ref = random_reference(rng, G)
    templates = []
    for _ in range(n_templates):
        length = rng.randint(1, min(max_len, G))
        templates.append((rng.randint(0, G - length), length))
    templates.append((0, rng.randint(1, min(max_len, G))))                # a read at site 1
    last = rng.randint(1, min(max_len, G))
    templates.append((G - last, last))                                    # ... and one ending at the last site
    # a few variants per template, drawn many times: equal reads are the rule
    variants = []
    for (start, length) in templates:
        for _ in range(rng.randint(1, 5)):
            s = list(ref[start:start + length])
            for j in range(length):
                u = rng.random()
                if u < p_sub:
                    s[j] = rng.choice("ACGT")
                elif u < p_sub + p_n:
                    s[j] = "N"
                elif u < p_sub + p_n + p_gap:
                    s[j] = "_"
            variants.append((start, "".join(s)))
    reads = []
    for i in range(n_reads):
        start, s = variants[rng.randrange(len(variants))] if rng.random() < 0.9 else variants[0]
        if rng.random() < 0.05:                                           # a private substitution
            j = rng.randrange(len(s))
            s = s[:j] + rng.choice("ACGTN_") + s[j + 1:]
        reads.append((f"r{i}", start, s))
    return ref, reads


def gen_sam(seed, G=200, n_lines=120, min_phred=20):
    """A reference and a SAM text whose mapped lines all parse: every CIGAR letter, soft clips at both ends, I next
    to D, lower-case and foreign bases, qualities around the cut-off, header / empty / unmapped lines in between,
    duplicated lines."""
    rng = random.Random(seed)
    ref = random_reference(rng, G)
    lines = ["@HD\tVN:1.6\tSO:coordinate", f"@SQ\tSN:ref\tLN:{G}"]
    made = []
    while len(made) < n_lines:
        if made and rng.random() < 0.4:
            made.append(rng.choice(made))
            continue
        ops, ref_len, q_len = [], 0, 0
        if rng.random() < 0.3:
            ops.append((rng.randint(1, 4), "H"))
        if rng.random() < 0.4:
            ops.append((rng.randint(1, 5), "S"))
        for _ in range(rng.randint(1, 5)):
            op = rng.choice("MMMM=XIDNP")
            n = rng.randint(1, 12) if op in "MX" else rng.randint(1, 3)
            ops.append((n, op))
        if rng.random() < 0.4:
            ops.append((rng.randint(1, 5), "S"))
        for n, op in ops:
            if op in "MXPDN":                                             # ('=' is no letter: its chunk is passed over)
                ref_len += n                                              # columns of the aligned string
            if op in "MXPISN":
                q_len += n                                                # what the reference's walk consumes of the query
        if ref_len == 0 or ref_len > G or q_len == 0:
            continue
        pos = rng.randint(1, G - ref_len + 1)
        seq = "".join(rng.choice("ACGTACGTACGTNacgtRY_") for _ in range(q_len))
        qual = "".join(chr(33 + rng.choice([min_phred - 1, min_phred, min_phred + 1, 40, 40, 40])) for _ in range(q_len + rng.randint(0, 2)))
        cigar = "".join(f"{n}{op}" for n, op in ops)
        flag = rng.choice([0, 16, 99, 147])
        made.append(f"q{len(made)}\t{flag}\tref\t{pos}\t60\t{cigar}\t*\t0\t0\t{seq}\t{qual}\tNM:i:0")
    for ln in made:
        lines.append(ln)
        u = rng.random()
        if u < 0.05:
            lines.append("")
        elif u < 0.12:
            lines.append(f"u{len(lines)}\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII")
    return ref, "\n".join(lines) + "\n"
