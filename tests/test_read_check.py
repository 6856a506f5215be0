"""The pure host logic of a host-buffer batch (wepp_amd/csrc/read_check.hpp) under AddressSanitizer + UBSan on the CPU:
tests/cxx/read_check_main.cpp -- the range check of the staging tasks against a naive one over every small batch and
sub-range, with and without staging; every offset staged and every read checked by exactly one task; every offset a
chunk's upload sends staged by a chunk the upload waits for (the chunk-boundary fault of round 3, as an invariant);
the cut of a batch into sub-batches, chunks and parts around 2^16, 2^19 and 2^21 reads."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "read_check_main.cpp"), os.path.join(ROOT, "wepp_amd", "csrc", "errors.cpp")]


def test_read_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "read_check_main")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                            *SRCS, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("no sanitizer runtime: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip().startswith("ok "), (run.stdout[-500:], run.stderr[-3000:])
