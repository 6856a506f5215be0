"""The group pass of place_dev.hpp without a GPU: tests/cxx/group_pass_emu.cpp runs pair_update -- the one statement of
the all-pairs arithmetic, shared by the 64-lane pass and the group pass -- in the loop of a group of 8 and of 16 lanes
over entry sets of 1 - 16 entries, against sorted_query for the same entries.  A program of its own, built plain and
with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_group_pairs_against_the_sorted_pass(tmp_path, flags):
    exe = str(tmp_path / "group_pass_emu")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-w", *flags, "-I", os.path.join(CXX, "hip_emu"),
                           os.path.join(CXX, "group_pass_emu.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:]
    m = re.search(r"sets=(\d+) g8=(\d+) g16=(\d+) shared_node=(\d+) shared_end=(\d+) node_at_end=(\d+) no_cut=(\d+) mismatches=0", run.stdout)
    assert m, run.stdout[-2000:]
    sets, g8, g16 = int(m.group(1)), int(m.group(2)), int(m.group(3))
    # every size 1 .. 16 by the wide group, 1 .. 8 by the narrow one as well
    assert g16 == sets and 0 < g8 < sets
