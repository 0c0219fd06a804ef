"""The seed index of the catalogue genotype on the CPU: mtr_amd/csrc/seed_index.h (the functions mtr_k_cat_scan runs per position, and the host's
side of the table) is built by the plain host C++ compiler into tests/seed_index_check.cpp, a program of its own that compares window codes,
filter and probe with brute force written there - every seed length 8..16, windows on every residue of a packed word, the last window of a
read, a read shorter than a seed, duplicate codes, a table filled to half, an empty table.  It is built twice: plain, and with the address and
undefined-behaviour sanitizers (no library is loaded into Python under a sanitizer: the check is a program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "seed_index_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_seed_index_against_brute_force(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "seed_index_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 10000
