"""What the known-motif locus search adds to the per-lane code, on the CPU: tests/motif_loci_check.cpp, a program of its own, holds the windowed
lane DP of mtr_amd/csrc/motif_dp.h (the functions mtr_k_motif_loci_lanes<UB> runs) to the unwindowed DP of the copied-out window - every phase
of the window's first base, windows that end on the read's last base, windows of one row, every bucket at both ends, 64 lanes of unequal windows
on one interleaved cell buffer - and the split rule and the length classes of mtr_amd/csrc/motif_loci.h to the definition written out naively.
It is built twice: plain, and with the address and undefined-behaviour sanitizers (no library is loaded into Python under a sanitizer)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "motif_loci_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_windowed_lane_dp_and_the_split_rule(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "motif_loci_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "windows checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    words = r.stdout.split()
    assert int(words[0]) > 5000 and int(words[words.index("splits") - 1]) > 100000
