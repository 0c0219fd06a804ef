"""What the device build of a prepared catalogue shares with the host, on the CPU: mtr_amd/csrc/catalog_build.h (the slots' codes and the
reverse complement, the sort's digit and stable rank, the duplicate drop, the table's sizes) is built by the plain host C++ compiler into
tests/catalog_build_check.cpp, a program of its own that runs the sort as the kernels do - a wavefront of emulated ballots a step - and
compares with std::stable_sort and brute force written there.  It is built twice: plain, and with the address and undefined-behaviour
sanitizers (no library is loaded into Python under a sanitizer: the check is a program with its own main)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "catalog_build_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_catalogue_build_helpers_against_brute_force(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "catalog_build_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "cases checked" in r.stdout and r.stdout.rstrip().endswith(": ok") and r.stderr == ""
    assert int(r.stdout.split()[0]) >= 3000
