"""The host-only code of wepp_epp_resolve under AddressSanitizer + UBSan on the CPU: the reader of
residual_mutations.txt, the checks on the residual list and its stable order by position
(tests/cxx/resolve_host_sanitized.cpp, a program of its own linked with the host sources it needs)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cxx", "resolve_host_sanitized.cpp"), os.path.join(ROOT, "wepp_amd", "host", "mat.cpp"),
        os.path.join(ROOT, "wepp_amd", "csrc", "errors.cpp")]


def test_residual_reader_and_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resolve_host_sanitized")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            *SRCS, "-lz", "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-500:], run.stderr[-3000:])
