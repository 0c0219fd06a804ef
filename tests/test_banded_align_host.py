"""The allele consensus' alignment on the CPU: mtr_amd/csrc/banded_align.h (the band, the cell and its direction rule, the anti-diagonal schedule
mtr_k_cons_align runs with a pair of diagonals per lane, the vote walk, the emission of a position) is built by the plain host C++ compiler into
tests/banded_align_check.cpp, a program of its own that compares D(n, m), every in-band cell's direction, the walk's votes and the emission with
a brute-force full matrix written there - over 10 000 seeded pairs of lengths 0..70, band_extra 0 / 1 / 8, length differences of either sign,
both layouts of the directions.  It is built twice: plain, and with the address and undefined-behaviour sanitizers (no library is loaded into
Python under a sanitizer: the check is a program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "banded_align_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_banded_alignment_against_brute_force(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "banded_align_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 10000
