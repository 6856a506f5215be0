"""The host side of a Fitch-Sankoff plan without a GPU (wepp_amd/csrc/fitch_plan.hpp: the form of a run, the chunk and
level tables, the shape of a run) and the two ways a device table is made (handle.hpp: DevMem::alloc, upload_whole):
tests/cxx/fitch_plan_main.cpp checks them against the emulated runtime of tests/cxx/hip_emu, built plain and under
AddressSanitizer + UBSan, a program of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "fitch_plan_main.cpp"), os.path.join(ROOT, "wepp_amd", "csrc", "errors.cpp")]


@pytest.mark.parametrize("how", ["plain", "sanitized"])
def test_fitch_plan_host(tmp_path, how):
    flags = ["-O1"]
    if how == "sanitized":
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        can = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if can.returncode != 0:
            pytest.skip("no sanitizer runtime: " + can.stderr[-200:])
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "fitch_plan_main")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", *flags, "-pthread", "-I", os.path.join(ROOT, "tests", "cxx", "hip_emu"),
                            *SRCS, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip().startswith("ok "), (run.stdout[-500:], run.stderr[-3000:])
