"""The split of the allele calls on the CPU: mtr_amd/csrc/allele_split.h (the functions mtr_k_allele_split runs, one share of a locus' splits per
lane) is built by the plain host C++ compiler into tests/allele_split_check.cpp, a program of its own that compares the medians, sad from the
prefix sums, "admissible" and the best split with brute force written there - over 10 000 seeded lists of 0..70 values (values in 0..5, two
noisy clusters, uniform in 0..833 333) under every combination of min_support 1 / 3, min_percent 0 / 20 / 50 and min_sep 1 / 5.  It is built
twice: plain, and with the address and undefined-behaviour sanitizers (no library is loaded into Python under a sanitizer: the check is a
program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "allele_split_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_split_against_brute_force(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "allele_split_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 10000
