"""The genotype quality's arithmetic on the CPU: mtr_amd/csrc/genotype_quality.h (the quality-weighted banded score in the schedule
mtr_k_gq_score runs - one alignment per wavefront, four side by side in the rows of one, two in its halves -, T, what an entry makes of its
scores and the locus' reduction) is built by the plain host C++ compiler into tests/genotype_quality_check.cpp, a program of its own that
compares it with a full matrix and a naive loop written there: more than 10 000 seeded pairs of lengths 0..70 at the borders of the kernels'
buckets, qualities 0..93 and none, and the definition's two properties.  It is built twice: plain, and with the address and
undefined-behaviour sanitizers (no library is loaded into Python under a sanitizer: the check is a program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "genotype_quality_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_score_the_table_and_the_locus_reduction_against_brute_force(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "genotype_quality_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 10000
