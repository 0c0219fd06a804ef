"""Which revisions Engine.test_revise takes (mtr_amd/csrc/revise_task.h: the bounds under which the batch path hands a record to its revision) on the
CPU: tests/revise_task_check.cpp moves one field of a batch-path task just past and just onto every bound and holds random tasks to a yes / no model
of the reference's conditions; it is built here by the host C++ compiler with the address and undefined-behaviour sanitizers, then run as a plain
child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_TASKS = 4000


def test_revise_task_bounds_against_the_model(tmp_path):
    # the sanitizers' runtimes are linked into the program itself (clang's default, g++ on request): it needs nothing loaded before it
    gxx, clang = shutil.which("g++"), shutil.which("clang++")
    assert gxx or clang, "no host C++ compiler"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang]
    exe = str(tmp_path / "revise_task_check")
    subprocess.run([*cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", exe, os.path.join(ROOT, "tests", "revise_task_check.cpp")], check=True)
    p = subprocess.run([exe, str(RANDOM_TASKS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.startswith(f"ok: 28 named cases, {RANDOM_TASKS} random tasks"), p.stdout


def test_the_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "mtr_amd", "csrc", "revise_task.h")).read()
    assert "hip_runtime" not in src and "hipMalloc" not in src and "__global__" not in src and "#include \"" not in src
