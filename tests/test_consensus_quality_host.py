"""The weighted vote's arithmetic on the CPU: mtr_amd/csrc/banded_align.h's baq_walk and baq_emit (what mtr_k_cq_align's lane 0 and mtr_k_cq_emit
run) are built by the plain host C++ compiler into tests/consensus_quality_check.cpp, a program of its own that compares them with a full-matrix
brute force written there from the header's words - every pair of the lengths of consensus_cases.LENGTHS, bands of 127 / 128 / 129 and 255 / 256
diagonals, qual_cap 1, 10, 40 and 93 - and, at qual_cap 1, with ba_walk and ba_emit.  It is built twice: plain, and with the address and
undefined-behaviour sanitizers (no library is loaded into Python under a sanitizer: the check is a program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "consensus_quality_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_weighted_walk_and_emission_against_brute_force(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "consensus_quality_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 5000


def test_the_program_uses_the_lengths_of_the_shared_cases():
    from tests import consensus_cases as cc

    assert "{ " + ", ".join(str(n) for n in cc.LENGTHS) + " }" in open(SRC).read()
