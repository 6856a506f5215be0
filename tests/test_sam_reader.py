"""The SAM parser of the host mirror (wepp_amd/host/sam_reader.cpp) through a program of its own
(tests/cxx/sam_reader_main.cpp) against tests/sam_model.py: the generator's SAM texts (plain and .gz) read alike, and
every refused input ends with the model's message.  The same program is built once more under AddressSanitizer + UBSan
and run stand-alone on the same inputs."""
import gzip
import os
import subprocess

import pytest

import sam_model as sm
from test_sam_model import line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "sam_reader_main.cpp"), os.path.join(ROOT, "wepp_amd", "host", "sam_reader.cpp"),
        os.path.join(ROOT, "wepp_amd", "host", "mat.cpp")]

REFUSED = [
    "q\t0\tref\t3\t60\t4M\t*\t0\t0\tACGT",
    line("4M", "ACGT", "*"),
    line("4M", "ACGT", "III"),
    line("5M", "ACGT"),
    line("4M", "ACGT", pos=0),
    line("4M", "ACGT", pos=8),
    line("4S", "ACGT"),
    line("*", "ACGT"),
    line("4M", "ACGT", pos="x"),
    line("4M", "ACGT", flag="f"),
    line("99999999999M", "ACGT"),
]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp(request.param) / "sam_reader_main")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else ["-O2"]
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, *SRCS, "-o", out, "-lz"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return out


def run(exe, path, genome, min_phred=20):
    return subprocess.run([exe, str(path), str(genome), str(min_phred)], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))


def test_generated_sam_texts(exe, tmp_path):
    for seed in range(6):
        ref, text = sm.gen_sam(seed, G=150 + 10 * seed, min_phred=15 + 3 * seed)
        want = sm.parse_sam(text, len(ref), 15 + 3 * seed)
        assert len(want) >= 100
        plain, gz = tmp_path / f"s{seed}.sam", tmp_path / f"s{seed}.sam.gz"
        plain.write_text(text)
        gz.write_bytes(gzip.compress(text.encode()))
        for path in (plain, gz):
            got = run(exe, path, len(ref), 15 + 3 * seed)
            assert got.returncode == 0, got.stderr[-2000:]
            rows = [tuple(r.split("\t")) for r in got.stdout.split("\n") if r]
            assert [(n, int(s), a) for n, s, a in rows] == want, (seed, path)


def test_line_ends_and_a_last_line_without_newline(exe, tmp_path):
    text = "@HD\tVN:1\r\n" + line("2M", "AC", name="a") + "\r\n" + line("2M1D1M", "GTA", name="b", pos=5)
    p = tmp_path / "crlf.sam"
    p.write_bytes(text.encode())
    got = run(exe, p, 10)
    assert got.returncode == 0 and got.stdout == "a\t2\tAC\nb\t4\tGT_A\n", (got.stdout, got.stderr)
    assert sm.parse_sam(text, 10) == [("a", 2, "AC"), ("b", 4, "GT_A")]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refused_inputs(exe, tmp_path, k):
    text = line("2M", "AC", name="ok") + "\n" + REFUSED[k] + "\n"
    with pytest.raises(sm.SamError) as ei:
        sm.parse_sam(text, 10)
    assert str(ei.value).startswith("line 2: ")
    p = tmp_path / "bad.sam"
    p.write_text(text)
    got = run(exe, p, 10)
    assert got.returncode == 2 and got.stderr.strip().split("\n")[-1] == str(ei.value), (got.stderr, str(ei.value))


def test_missing_file(exe, tmp_path):
    got = run(exe, tmp_path / "none.sam", 10)
    assert got.returncode == 2 and "Could not open the SAM file" in got.stderr
