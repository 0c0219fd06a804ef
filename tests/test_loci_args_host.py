"""What the loci's text and lengths decide (mtr_amd/csrc/loci_args.h: the checks of the genotype calls and of mtr_catalog_create with their words,
the arrays of lengths, the codes of flanks and motifs) on the CPU: tests/loci_args_check.cpp holds a sequential model of the checks' order and
brute-force constructions of the arrays, and is built here by the host C++ compiler with the address and undefined-behaviour sanitizers, then
run as a plain child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_CATALOGUES = 400


def test_loci_args_against_the_sequential_model(tmp_path):
    # the sanitizers' runtimes are linked into the program itself (clang's default, g++ on request): it needs nothing loaded before it
    gxx, clang = shutil.which("g++"), shutil.which("clang++")
    assert gxx or clang, "no host C++ compiler"
    cxx = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [clang]
    exe = str(tmp_path / "loci_args_check")
    subprocess.run([*cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", exe, os.path.join(ROOT, "tests", "loci_args_check.cpp")], check=True)
    p = subprocess.run([exe, str(RANDOM_CATALOGUES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.startswith(f"ok: 19 named cases, {RANDOM_CATALOGUES} random catalogues"), p.stdout


def test_the_header_is_free_of_hip():
    # the header and all it includes; dp_task_plan.h (tests/test_dp_task_plan_host.py) and what it adds to them
    for name in ("loci_args.h", "mtr_common.h", "catalog_build.h", "flank_bv.h", "motif_dp.h", "seed_index.h", "dp_task_plan.h", "motif_loci.h"):
        src = open(os.path.join(ROOT, "mtr_amd", "csrc", name)).read()
        assert "hip_runtime" not in src and "hipMalloc" not in src and "__global__" not in src, name
