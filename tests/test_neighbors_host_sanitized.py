"""The host-only code of the neighbour sets under AddressSanitizer + UBSan on the CPU: score_comparator, the ranking
and truncation of a region and the union over a selection (tests/cxx/neighbors_host_sanitized.cpp, a program of its
own over wepp_amd/host/neighbor_rank.hpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "neighbors_host_sanitized.cpp")]


def test_ranking_and_union_under_sanitizers(tmp_path):
    exe = str(tmp_path / "neighbors_host_sanitized")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            *SRCS, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-500:], run.stderr[-3000:])
