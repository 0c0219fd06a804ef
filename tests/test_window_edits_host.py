"""The window edits' sequential functions (mtr_amd/csrc/window_edits.h: the code the gfx950 lanes run) on the CPU: tests/window_edits_check.cpp holds
we_rows and we_walk to a brute-force full matrix with stored predecessors, the path read forward.  Built here by the host C++ compiler, plain and
with the address and undefined-behaviour sanitizers linked into the program itself, and run as a plain child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 12000


def _build(tmp_path, name, sanitize):
    # the sanitizers' runtimes are linked into the program itself (clang's default, g++ on request): it needs nothing loaded before it
    gxx, clang = shutil.which("g++"), shutil.which("clang++")
    assert gxx or clang, "no host C++ compiler"
    cxx = ([gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang]) if sanitize else [gxx or clang]
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    exe = str(tmp_path / (name + ("_san" if sanitize else "")))
    subprocess.run([*cxx, "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")], check=True)
    return exe


@pytest.mark.parametrize("sanitize", (False, True))
def test_the_rows_and_the_walk_against_the_brute_force_matrix(tmp_path, sanitize):
    p = subprocess.run([_build(tmp_path, "window_edits_check", sanitize), str(CASES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    head, runs = p.stdout.split(",")[:2]
    assert head == f"ok: {CASES} cases" and int(runs.split()[0]) >= 10000, p.stdout


def test_the_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "mtr_amd", "csrc", "window_edits.h")).read()
    assert "hip_runtime" not in src and "hipMalloc" not in src and "__global__" not in src
