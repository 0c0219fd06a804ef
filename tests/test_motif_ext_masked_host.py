"""The masked rows of the per-lane anchored extension on the CPU: mtr_amd/csrc/motif_ext.h's motif_ext_rows<UB, false> - what mtr_k_ptc_ext<UB>
runs, one task per lane with the lane's own motif, length and direction - is built by the plain host C++ compiler into
tests/motif_ext_masked_check.cpp, a program of its own that compares it with the rows compiled without a cut where U == UB and with a full-matrix
DP for every U <= UB - both directions, every bucket, lo and hi at all 16 residues of a word, six score sets, the packed text sized to the window
so that a load beyond it trips.  It is built twice: plain, and with the address and undefined-behaviour sanitizers (no library is loaded into
Python under a sanitizer: the check is a program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "motif_ext_masked_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_masked_rows_against_the_uncut_rows_and_a_full_matrix_dp(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "motif_ext_masked_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 10000 and int(r.stdout.split("(")[1].split()[0]) >= 4000
