"""The per-unit function of the motif catalogue on the CPU: mtr_amd/csrc/unit_motif.h (the function mtr_k_unit_motif runs, one lane per unit)
is built by the plain host C++ compiler (tests/unit_motif_check.cpp) and compared with the brute force of tests/unit_motif_ref.py - the
minimum over all 2p rotations, the smallest divisor - on every string of length 1..8, on random non-primitive units up to 500 bases and on
the edges of the length range.  mtr_amd.canonical_motif, the pure-Python function of the package, is held to the same brute force.
The same .cpp, built as a program of its own with the address and undefined-behaviour sanitizers, checks itself against a C++ brute force."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import mtr_amd
from tests import unit_motif_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "unit_motif_check.cpp")


@pytest.fixture(scope="module")
def um(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    lib = str(tmp_path_factory.mktemp("um") / "libunit_motif_check.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", lib, SRC], check=True)
    h = C.CDLL(lib)
    h.um_check_units.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    h.um_check_units.restype = None
    return h


def _header(um, units, slots=1024):
    """-> per unit (motif, strand, rotation, motif_len), the hashes, the start slots"""
    n = len(units)
    data = np.frombuffer(b"".join(units) + b"\0", np.uint8)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(u) for u in units])
    strand, rotation, motif_len = (np.full(n, -1, np.int32) for _ in range(3))
    motifs = np.full(len(data), 0xee, np.uint8)
    hashes, start = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    um.um_check_units(data.ctypes.data, off.ctypes.data, n, strand.ctypes.data, rotation.ctypes.data, motif_len.ctypes.data, motifs.ctypes.data,
                      hashes.ctypes.data, slots, start.ctypes.data)
    mb = motifs.tobytes()
    out = []
    for k in range(n):
        d = int(motif_len[k])
        assert 0 <= d <= len(units[k])
        assert mb[int(off[k]) + d:int(off[k + 1])] == b"\xee" * (len(units[k]) - d), "the motif's bytes alone are written"
        out.append((mb[int(off[k]):int(off[k]) + d], int(strand[k]), int(rotation[k]), d))
    return out, hashes, start


def _compare(um, units):
    got, hashes, start = _header(um, units)
    for u, g, h, s in zip(units, got, hashes, start):
        want = ref.brute(u)
        assert g == want, (u if len(u) < 80 else (len(u), u[:40]), g[1:], want[1:])
        assert g[2] < max(g[3], 1)
        assert int(h) == ref.motif_hash(want[0]) and int(s) == ref.start_slot(want[0], 1024)
    return got


def test_every_string_up_to_length_8(um):
    units = [bytes(t) for p in range(1, 9) for t in itertools.product(b"ACGT", repeat=p)]
    assert len(units) == 87380
    got = _compare(um, units)
    assert sum(1 for g in got if g[1] == 1) > 10000 and sum(1 for u, g in zip(units, got) if g[3] < len(u)) > 300


def test_worked_values_and_the_empty_unit(um):
    got, _, _ = _header(um, [u for u, *_ in ref.WORKED] + [b""])
    assert got[:-1] == [w[1:] for w in ref.WORKED]
    assert got[-1] == (b"", 0, 0, 0)
    for u, *want in ref.WORKED:
        assert ref.brute(u) == tuple(want)


def test_random_non_primitive_units_up_to_500_bases(um):
    rng = np.random.RandomState(20270)
    units = ref.random_units(rng, 300)
    got = _compare(um, units)
    assert sum(1 for u, g in zip(units, got) if g[3] < len(u)) > 100 and max(len(u) for u in units) > 450


def test_the_edges_of_the_length_range(um):
    rng = np.random.RandomState(20271)
    units = []
    for p in (63, 64, 65, 499, 500):
        units.append(bytes(b"ACGT"[c] for c in rng.randint(0, 4, size=p)))
        units.append(bytes(b"AC"[c] for c in rng.randint(0, 2, size=p)))              # long runs of equal comparisons
        units.append(bytes(b"ACGT"[c] for c in rng.randint(0, 4, size=p)).replace(b"A", b"C"))     # no A: the least base is not the alphabet's
    units += [b"T" * 499 + b"A", b"A" * 500, b"T" * 500, b"A" * 499 + b"C", b"AC" * 250, b"CA" * 250, (b"A" * 249 + b"C") * 2, b"TG" * 249 + b"T"]
    got = _compare(um, units)
    assert got[units.index(b"T" * 499 + b"A")] == (b"A" * 499 + b"T", 1, 1, 500)
    assert got[units.index(b"A" * 500)] == (b"A", 0, 0, 1) and got[units.index(b"T" * 500)] == (b"A", 1, 0, 1)
    assert got[units.index(b"CA" * 250)] == (b"AC", 0, 1, 2)


def test_canonical_motif_is_the_same_function():
    rng = np.random.RandomState(20272)
    units = [bytes(t) for p in range(1, 7) for t in itertools.product(b"ACGT", repeat=p)] + ref.random_units(rng, 60) + [b"", b"T" * 499 + b"A", b"A" * 500]
    for u in units:
        motif, strand, rotation, _ = ref.brute(u)
        assert mtr_amd.canonical_motif(u) == (motif, strand, rotation), u
    assert mtr_amd.canonical_motif("CTG") == ("AGC", 1, 1) and mtr_amd.canonical_motif("") == ("", 0, 0)
    assert mtr_amd.canonical_motif(bytearray(b"GT")) == (b"AC", 1, 0)


def test_the_header_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """no library is loaded into Python under a sanitizer: the check is a program with its own main"""
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "unit_motif_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DUNIT_MOTIF_MAIN", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "units checked: ok" in r.stdout and r.stderr == ""
