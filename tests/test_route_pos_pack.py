"""The pack / unpack pair of k_route's word per position (wepp_amd/csrc/route_pos.hpp) on the host, for length fields of
24 bits (the product) and 3 bits (the rtlen3 test build): round trip, saturation, recognition of a saturated field
(tests/cxx/route_pos_pack_main.cpp, a program of its own), plain and under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "route_pos_pack_main.cpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("flags", [["-O2"], SANITIZE], ids=["plain", "sanitized"])
@pytest.mark.parametrize("bits", [24, 3])
def test_route_pos_pack(tmp_path, bits, flags):
    exe = str(tmp_path / "route_pos_pack")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, f"-DWEPP_RT_LEN_BITS={bits}", SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip() == f"ok {bits}", (run.stdout[-500:], run.stderr[-3000:])
