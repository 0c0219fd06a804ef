"""The layouts and sizes the hosts of the wrap-around DP kernels hand to the device (mtr_amd/csrc/dp_task_plan.h: the seven-column task table, the
scratch of a code matrix, the lane slots, the five-launch plan of the known-motif kernels, a round of the locus search) on the CPU: tests/dp_task_plan_check.cpp writes the
table through in a buffer of exactly the ints the hosts allocate and restates the two hosts' formulas one statement after the other, and is built
here by the host C++ compiler with the address and undefined-behaviour sanitizers, then run as a plain child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_SHAPES = 300


def test_dp_task_plan_against_the_sequential_formulas(tmp_path):
    # the sanitizers' runtimes are linked into the program itself (clang's default, g++ on request): it needs nothing loaded before it
    gxx, clang = shutil.which("g++"), shutil.which("clang++")
    assert gxx or clang, "no host C++ compiler"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang]
    exe = str(tmp_path / "dp_task_plan_check")
    subprocess.run([*cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", exe, os.path.join(ROOT, "tests", "dp_task_plan_check.cpp")], check=True)
    p = subprocess.run([exe, str(RANDOM_SHAPES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.startswith(f"ok: 81 named cases, {RANDOM_SHAPES} random shapes"), p.stdout
