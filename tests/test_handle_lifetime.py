"""What a handle owns goes with it (wepp_amd/csrc/handle.hpp), under AddressSanitizer + UBSan on the CPU:
tests/cxx/handle_lifetime_main.cpp builds handles against the emulated runtime of tests/cxx/hip_emu, whose streams and
events are heap tokens and which counts what is alive -- a handle deleted as it was made, one that holds every buffer,
stream and event it can (the grow-only buffers made, regrown and asked for less), and the handle's own set-up stopped
at each of its device allocations in turn: nothing is left, nothing is freed twice."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "handle_lifetime_main.cpp"), os.path.join(ROOT, "wepp_amd", "csrc", "errors.cpp")]


def test_handle_lifetime_under_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if can.returncode != 0:
        pytest.skip("no sanitizer runtime: " + can.stderr[-200:])
    exe = str(tmp_path / "handle_lifetime_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-pthread", "-I", os.path.join(ROOT, "tests", "cxx", "hip_emu"), *SRCS, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip().startswith("ok "), (run.stdout[-500:], run.stderr[-3000:])
