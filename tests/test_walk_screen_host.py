"""The dead-range screen of the staged unit search, range by range on the CPU: the per-range function of mtr_amd/csrc/walk_screen.h (the one
mtr_k_walk_screen runs, one lane per range) is built by the plain host C++ compiler (tests/walk_screen_check.cpp) and compared with the CPU
oracle's search_unit on every candidate range of 200 headline reads and on crafted ranges (tests/walk_screen_cases.py).

What is asserted per range that the rule covers (w < 1000 and at most 64 bases):
  1. max_freq equals the oracle's max_freq of the window's k = 2 table;
  2. dead  <=>  max_freq <= 5 and max_freq + n_raw(k) <= 5 for every larger k of the window (the oracle's max_freq, n_raw worked out here):
     the condition under which the kernels before the screen ended with no candidate and no k left to search;
  3. dead  ==>  the oracle's search_unit returns no unit (found = 0, no period) at EVERY k of the window's k range.
The converse of 3 does not hold and is not asserted: a range whose most frequent 2-mer node is seen exactly five times, or more often, is not dead
by the rule - its larger k are searched as before - and most such ranges yield no unit either ((AC)x5 is one: AC five times, no seed at any k).
The test prints how many of the headline's ranges are of that kind (200 reads: 43 708 candidate ranges, 40 576 covered by the rule, 31 831 dead,
4 816 covered, not dead and without a unit at any k)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mtr_amd import synth
from tests import walk_screen_cases as cases
from tests.oracle_binding import Oracle, OSearchResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_NUM_FREQ_UNIT = 5


@pytest.fixture(scope="module")
def ws(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    lib = str(tmp_path_factory.mktemp("ws") / "libwalk_screen_check.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", lib,
                    os.path.join(ROOT, "tests", "walk_screen_check.cpp")], check=True)
    h = C.CDLL(lib)
    h.ws_check_ranges.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    h.ws_check_ranges.restype = None
    h.ws_k_range.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    h.ws_k_range.restype = None
    return h


@pytest.fixture(scope="module")
def oracle():
    o = Oracle()
    yield o
    o.close()


def _screen(ws, codes, ranges):
    pk = cases.pack(codes)
    r = np.asarray(ranges, np.int32).reshape(-1, 3)
    qs, qe, w = (np.ascontiguousarray(r[:, i]) for i in range(3))
    n = len(r)
    applies, max_freq, dead = (np.zeros(n, np.int32) for _ in range(3))
    ws.ws_check_ranges(pk.ctypes.data, len(codes), n, qs.ctypes.data, qe.ctypes.data, w.ctypes.data,
                       applies.ctypes.data, max_freq.ctypes.data, dead.ctypes.data)
    return applies, max_freq, dead


def _k_range(ws, w):
    a, b = C.c_int32(), C.c_int32()
    ws.ws_k_range(w, C.byref(a), C.byref(b))
    return a.value, b.value


def _no_unit_at_any_k(oracle, codes, qs, qe, k_lo, k_hi, res):
    for k in range(k_lo, k_hi + 1):
        found = oracle.lib.mtro_search_unit(oracle.h, codes.ctypes.data, len(codes), qs, qe, k, C.byref(res))
        assert found >= 0
        if found or res.period > 0:
            return False
    return True


def _check_read(ws, oracle, codes, ranges, name):
    """-> (ranges the rule covers, dead ones, covered ranges that are not dead and yield no unit at any k)"""
    codes = np.ascontiguousarray(codes, np.uint8)
    L = len(codes)
    applies, max_freq, dead = _screen(ws, codes, ranges)
    res = OSearchResult()
    n_cov = n_dead = n_idle = 0
    for i, (qs, qe, w) in enumerate(ranges):
        want_applies = w < 1000 and qe - qs + 1 <= 64                     # the issue's rule, restated: the test includes a case exactly then
        assert bool(applies[i]) == want_applies, (name, qs, qe, w)
        if not want_applies:
            assert max_freq[i] == -1 and dead[i] == -1
            continue
        n_cov += 1
        k_lo, k_hi = _k_range(ws, w)
        assert k_lo == 2 and k_hi == (10 if w < 100 else 12), (w, k_lo, k_hi)
        mf = oracle.search_unit(codes, qs, qe, 2)["max_freq"]
        assert max_freq[i] == mf, (name, qs, qe, w, int(max_freq[i]), mf)
        want_dead = mf <= MIN_NUM_FREQ_UNIT and all(mf + (qe - min(qe, L - k + 1) + 1) <= MIN_NUM_FREQ_UNIT for k in range(3, k_hi + 1))
        assert bool(dead[i]) == want_dead, (name, qs, qe, w, mf)
        no_unit = _no_unit_at_any_k(oracle, codes, qs, qe, k_lo, k_hi, res)
        if dead[i]:
            n_dead += 1
            assert no_unit, (name, qs, qe, w, mf)
        elif no_unit:
            n_idle += 1
    return n_cov, n_dead, n_idle


def test_crafted_ranges(ws, oracle):
    seen = {}
    for name, codes, ranges in cases.crafted():
        n_cov, n_dead, _ = _check_read(ws, oracle, codes, ranges, name)
        seen[name] = (len(ranges), n_cov, n_dead)
    # the cases say what they were made for
    by = {name: (codes, ranges) for name, codes, ranges in cases.crafted()}

    def one(name, r):
        codes, _ = by[name]
        a, mf, d = _screen(ws, codes, [r])
        return int(a[0]), int(mf[0]), int(d[0])
    assert one("ac_x5", (50, 60, 5)) == (1, 5, 0)                         # AC five times: no seed at k = 2, but the bound leaves k = 3 alive
    assert one("ac_x5", (50, 59, 5)) == (1, 6, 0)                         # the window's last base, a raw C, counts as the 2-mer AC
    assert one("ac_x6", (50, 62, 5))[1] == 6 and one("ac_x6", (50, 61, 5))[1] == 7
    assert one("a_x6", (50, 55, 5)) == (1, 6, 0)                          # AA five times and the window's last base, a raw A, counted as AA
    assert one("t_x6", (50, 55, 5))[1] == 5                               # TT five times; the raw T counts as the 2-mer AT
    assert one("a_x7", (50, 56, 5))[1] == 7
    assert one("acg_x22", (50, 113, 5))[0] == 1 and one("acg_x22", (50, 114, 5)) == (0, -1, -1)      # 64 bases / 65 bases
    assert one("w_1280_over_a_short_window", (10, 30, 1280)) == (0, -1, -1) and one("w_1280_over_a_short_window", (10, 30, 640))[0] == 1
    assert one("windows_of_5_and_6", (10, 14, 5))[0] == 1 and one("windows_of_5_and_6", (10, 15, 5))[0] == 1
    assert any(n_dead > 0 for _, _, n_dead in seen.values()) and any(n_cov > n_dead for _, n_cov, n_dead in seen.values())


def test_every_candidate_range_of_200_headline_reads(ws, oracle):
    reads = [c for _, c in synth.make_reads("headline2k", 200, 2)]
    n_all = n_cov = n_dead = n_idle = 0
    for i, codes in enumerate(reads):
        ranges = [(s, e, w) for s, e, w, _ in oracle.ranges(codes)]
        covered = [r for r in ranges if r[2] < 1000 and r[1] - r[0] + 1 <= 64]
        n_all += len(ranges)
        c, d, idle = _check_read(ws, oracle, codes, covered, f"headline2k read {i}")
        n_cov += c; n_dead += d; n_idle += idle
    print(f"headline2k, 200 reads: {n_all} candidate ranges, {n_cov} covered by the rule, {n_dead} dead ({n_dead / n_all:.1%} of all), "
          f"{n_idle} covered, not dead and without a unit at any k")
    # what the screen was built for: four ranges in five of this workload are dead (measured: 78 %)
    assert n_dead >= 0.70 * n_all, (n_dead, n_all)
