"""The file state of file-order mode (mtr_amd/csrc/file_state.h: the staircase, the one walk over it, the planning of both feeds) on the CPU:
tests/file_state_check.cpp holds a brute-force model of the reference's two whole-file buffers and is built here by the host C++ compiler with
the address and undefined-behaviour sanitizers, then run as a plain child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_FILES = 200
# A 720000-base read costs the model a million entries, and the sanitized build makes each slow: the first LONG_FILES of the random files get
# one each (the fixed file TAIL_LENS has one more); every other length class is drawn in all of them.
LONG_FILES = 6


def test_file_state_against_the_two_buffer_model(tmp_path):
    # the sanitizers' runtimes are linked into the program itself (clang's default, g++ on request): it needs nothing loaded before it
    gxx, clang = shutil.which("g++"), shutil.which("clang++")
    assert gxx or clang, "no host C++ compiler"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang]
    exe = str(tmp_path / "file_state_check")
    subprocess.run([*cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", exe, os.path.join(ROOT, "tests", "file_state_check.cpp")], check=True)
    p = subprocess.run([exe, str(RANDOM_FILES), str(LONG_FILES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.startswith(f"ok: 2 fixed files, {RANDOM_FILES} random files ({LONG_FILES} with a 720000-base read)"), p.stdout


def test_the_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "mtr_amd", "csrc", "file_state.h")).read()
    assert "hip_runtime" not in src and "hipMalloc" not in src and "__global__" not in src
