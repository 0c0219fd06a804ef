"""polish_repeat as a plan over the flagged positions (mtr_amd/csrc/polish_plan.h), on the CPU: the header the kernels compile is built by the
plain host C++ compiler (tests/polish_plan_check.cpp) and held

  1. to the CPU oracle on every polish_repeat call (G3p capture line) of 300 headline2k reads, seed 2: unit, node frequencies, k, rep_start and
     rep_end in, the k-mer table a plain map over win_node of the window; the polished unit must equal the line's `out` in every call;
  2. to the reference's walk over every position, compiled from the same header (the loop the kernels run under -DMTR_POLISH_WALK_ALL), on the
     crafted calls of tests/polish_cases.py - each also asserted to exercise what it was made for - and call for call on 20 000 random
     (unit, scores, k) triples with about a tenth of the positions flagged;
  3. the same random comparison once more in a stand-alone program built with -fsanitize=address,undefined and run directly.

Measured on the 1 357 calls of (1): 636 without a flagged position (one more with period <= k), 88 with one, 161 with 2-3, 135 with 4-8, 336
with more; 179 calls change the unit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import polish_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "polish_plan_check.cpp")


@pytest.fixture(scope="module")
def pp(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    lib = str(tmp_path_factory.mktemp("pp") / "libpolish_plan_check.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", lib, SRC], check=True)
    h = C.CDLL(lib)
    h.pp_check_polish.argtypes = [C.c_int32, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p] * 4
    h.pp_check_polish.restype = C.c_int32
    h.pp_random_compare.argtypes = [C.c_int32, C.c_uint64, C.c_void_p]
    h.pp_random_compare.restype = None
    return h


def polish(pp, walk_all, pk, L, rep_start, rep_end, k, unit, score):
    """-> (polished unit, info[8] of polish_plan_check.cpp: flagged, int_unit[-1] reads, altered, overflowed, look-ups, copied, through the body, table built)"""
    unit = np.ascontiguousarray(unit, np.uint8)
    score = np.ascontiguousarray(score, np.int32)
    out, info = np.zeros(cases.MAX_PERIOD, np.uint8), np.zeros(8, np.int32)
    n = pp.pp_check_polish(walk_all, pk.ctypes.data, L, rep_start, rep_end, k, len(unit), unit.ctypes.data, score.ctypes.data, out.ctypes.data, info.ctypes.data)
    return out[:n].copy(), [int(v) for v in info]


def test_crafted_calls_plan_equals_the_walk_over_every_position(pp):
    seen = set()
    for c in cases.crafted():
        pk, L = cases.pack(c["read"]), len(c["read"])
        args = (pk, L, c["rep_start"], c["rep_end"], c["k"], c["unit"], c["score"])
        out_all, info_all = polish(pp, 1, *args)
        out_plan, info_plan = polish(pp, 0, *args)
        assert out_plan.tolist() == out_all.tolist(), c["name"]
        assert info_plan[:4] == info_all[:4] and info_plan[7] == info_all[7], (c["name"], info_plan, info_all)       # flagged, H10 reads, altered, overflow, table
        assert info_all[3] or info_plan[5] + info_plan[6] == info_all[6], (c["name"], info_plan, info_all)            # every emission, copied or through the body
        # what the case was made for, on the walk over every position
        U, k, want = len(c["unit"]), c["k"], c["want"]
        flagged, undefined, altered, overflow, _, _, _, table = info_all
        if "altered" in want:
            assert altered
        if "unchanged" in want:
            assert not altered and out_all.tolist() == c["unit"].tolist()
        if "undefined" in want:
            assert undefined > 0
        if "overflow" in want:
            assert overflow and out_all.tolist() == c["unit"].tolist()
        else:
            assert not overflow
        if "longer" in want:
            assert len(out_all) > U
        if "shorter" in want:
            assert len(out_all) < U
        if "no_table" in want:
            assert not table and (U <= k or flagged == 0)
        if "flag_in_first_k" in want:
            sc = np.clip(c["score"], 0, 3)
            assert any(sc[j] == 1 and 0.8 * (k - 1) < sum(1 for i in range(min(k - 1, j + 1)) if sc[j - i] < 2) for j in range(k - 1))
        if "dirty_flag" in want:           # two substitutions closer than k, both taken: the lower one is met before the node is the unit's own again
            subs = sorted(p for p, kind in c["edits"] if kind == "sub")
            assert len(out_all) == U and any(b - a < k - 1 and out_all[a] != c["unit"][a] and out_all[b] != c["unit"][b] for a, b in zip(subs, subs[1:]))
        seen |= want
    assert seen >= {"altered", "unchanged", "undefined", "flag_in_first_k", "dirty_flag", "longer", "shorter", "overflow", "no_table"}
    assert {len(c["unit"]) for c in cases.crafted()} >= {6, 63, 64, 65, 128, 129, 499}
    assert {c["k"] for c in cases.crafted()} >= {2, 6, 7, 10, 11, 12}


def test_every_polish_call_of_300_headline_reads_equals_the_oracle(pp):
    reads, calls = cases.oracle_g3p("headline2k", 300, 2)
    assert len(calls) == 1357
    packed = {}
    hist = {"period <= k": 0, "0": 0, "1": 0, "2-3": 0, "4-8": 0, "more": 0}
    changed = 0
    for i, g in enumerate(calls):
        rd = g["rd"]
        if rd not in packed:
            packed[rd] = cases.pack(reads[rd])
        args = (packed[rd], len(reads[rd]), g["rep_start"], g["rep_end"], g["k"], g["unit"], g["score"])
        out, info = polish(pp, 0, *args)
        assert out.tolist() == g["out"].tolist(), (i, rd, g["rep_start"], g["rep_end"], g["k"], info)
        out_all, _ = polish(pp, 1, *args)
        assert out_all.tolist() == g["out"].tolist(), (i, "the walk over every position", rd, g["rep_start"], g["rep_end"], g["k"])
        f = info[0]
        hist["period <= k" if len(g["unit"]) <= g["k"] else "0" if f == 0 else "1" if f == 1 else "2-3" if f <= 3 else "4-8" if f <= 8 else "more"] += 1
        changed += out.tolist() != g["unit"].tolist()
    print(f"headline2k, 300 reads: {len(calls)} polish calls by flagged positions: {hist}; {changed} change the unit")
    assert changed > 100 and hist["0"] > 400 and hist["more"] > 200             # the census the plan was built on: most calls have none or many


def test_random_triples_plan_equals_the_walk_over_every_position(pp):
    s = np.zeros(10, np.int64)
    pp.pp_random_compare(20000, 1, s.ctypes.data)
    calls, differ, positions, flagged, altered, length_changed, overflowed, undefined = (int(v) for v in s[:8])
    print(f"{calls} random calls: {flagged / positions:.1%} of {positions} positions flagged, {altered} calls altered, {length_changed} changed "
          f"length, {overflowed} overflowed, {undefined} int_unit[-1] reads; look-ups plan {int(s[8])}, every position {int(s[9])}")
    assert calls == 20000 and differ == 0
    assert 0.05 < flagged / positions < 0.20                                    # about a tenth
    assert altered > 2000 and length_changed > 1000 and overflowed > 100 and undefined > 100


def test_random_triples_in_a_sanitized_program(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "polish_plan_check_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-DPOLISH_PLAN_CHECK_MAIN", "-o", exe, SRC], check=True)
    p = subprocess.run([exe, "20000", "2"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " differ 0 " in p.stdout, p.stdout
