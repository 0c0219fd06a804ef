"""The per-lane DP of the known-motif search on the CPU: mtr_amd/csrc/motif_dp.h (the functions mtr_k_motif_lanes<UB> runs, one read per lane)
is built by the plain host C++ compiler into tests/motif_dp_check.cpp, a program of its own that compares all nine outputs with a naive
full-matrix DP written there - every bucket at its smallest and largest U, L = 1, motifs that end inside a four-column dword, and groups of
64 lanes of unequal length on one interleaved cell buffer.  It is built twice: plain, and with the address and undefined-behaviour
sanitizers (no library is loaded into Python under a sanitizer: the check is a program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "motif_dp_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_lane_dp_against_a_full_matrix_dp(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "motif_dp_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "alignments checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) > 10000
