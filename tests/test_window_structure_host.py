"""The window structure's sequential function (mtr_amd/csrc/window_structure.h: the code the gfx950 lanes run) and the checks of the call's host
arguments (mtr_amd/csrc/window_structure_args.h) on the CPU: tests/window_structure_check.cpp holds ws_rows to a brute-force full matrix with
stored predecessors, rows iterated to their fixpoint; tests/window_structure_args_check.cpp holds the checks to a sequential model.  Both are
built here by the host C++ compiler, plain and with the address and undefined-behaviour sanitizers, and run as plain child processes."""
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
def test_the_lanes_function_against_the_brute_force_matrix(tmp_path, sanitize):
    p = subprocess.run([_build(tmp_path, "window_structure_check", sanitize), str(CASES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    head, runs = p.stdout.split(",")[:2]
    assert head == f"ok: {CASES} cases" and int(runs.split()[0]) >= 10000, p.stdout


@pytest.mark.parametrize("sanitize", (False, True))
def test_the_argument_checks_against_the_sequential_model(tmp_path, sanitize):
    p = subprocess.run([_build(tmp_path, "window_structure_args_check", sanitize), "400"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.startswith("ok: 16 named cases, 400 random sets of structures"), p.stdout


def test_the_headers_are_free_of_hip():
    for name in ("window_structure.h", "window_structure_args.h"):
        src = open(os.path.join(ROOT, "mtr_amd", "csrc", name)).read()
        assert "hip_runtime" not in src and "hipMalloc" not in src and "__global__" not in src, name
