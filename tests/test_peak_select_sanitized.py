"""The host-only choices of the peak loop under AddressSanitizer + UBSan on the CPU: the order of a tie group, the walk
that accepts peaks (tie group smaller than / equal to / larger than top_n, the max_peaks cut inside a group, everything
rejected but the first, equal ranks) and the stop rules (tests/cxx/peak_select_sanitized.cpp, a program of its own over
wepp_amd/host/peak_select.hpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "peak_select_sanitized.cpp")]


def test_peak_selection_under_sanitizers(tmp_path):
    exe = str(tmp_path / "peak_select_sanitized")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            *SRCS, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-500:], run.stderr[-3000:])
