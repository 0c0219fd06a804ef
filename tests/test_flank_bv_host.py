"""The per-lane scan of the flank search on the CPU: mtr_amd/csrc/flank_bv.h (the functions mtr_k_flank_lanes<W> runs, one read per lane) is built
by the plain host C++ compiler into tests/flank_bv_check.cpp, a program of its own that compares dist, end and start with full-matrix DPs
written there - both words, patterns of 1, 2, 31, 32, 33, 63 and 64 bases, texts of 0 and 1 bases, texts shorter than the pattern, the packed
words' edges, hits on the first and on the last base, two hits of equal distance, windows that begin inside a word.  It is built twice: plain,
and with the address and undefined-behaviour sanitizers (no library is loaded into Python under a sanitizer: the check is a program with its
own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "flank_bv_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_lane_scan_against_full_matrix_dps(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "flank_bv_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 10000
