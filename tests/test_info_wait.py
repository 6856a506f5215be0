"""The host's wait for the routing counters k_step reports (wepp_amd/csrc/info_wait.hpp: a function of "read the word",
"query the stream" and "now") without a GPU: the word at once, behind the yield threshold, behind the first queries;
never, with the stream complete (lost) or in error (that error); the previous call's word is not this call's
(tests/cxx/info_wait_main.cpp, a program of its own), plain and under AddressSanitizer + UBSan.  This is the only place
where a report that never comes is exercised: no GPU test provokes one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "info_wait_main.cpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("flags", [["-O2"], SANITIZE], ids=["plain", "sanitized"])
def test_info_wait(tmp_path, flags):
    exe = str(tmp_path / "info_wait")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread", *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-500:], run.stderr[-3000:])
