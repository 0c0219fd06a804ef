"""The sequence allele calls' arithmetic on the CPU: mtr_amd/csrc/seq_calls.h (the saturated banded distance in the schedule mtr_k_seq_dist runs -
one alignment per wavefront, and four side by side in the rows of one - the pair index, the medoid selection, the partition) is built by the
plain host C++ compiler into tests/seq_calls_check.cpp, a program of its own that compares it with a full-matrix Levenshtein and a naive triple
loop written there: more than 10 000 seeded pairs of lengths 0..70, K in {0, 1, 5, 31, 32, 254}, length differences of either sign with
|difference| = K and K + 1 among them.  It is built twice: plain, and with the address and undefined-behaviour sanitizers (no library is loaded
into Python under a sanitizer: the check is a program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "seq_calls_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_distance_the_pair_index_and_the_split_against_brute_force(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "seq_calls_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 10000
