"""ctypes binding of oracle/liboracle_mtr.so — TEST INFRASTRUCTURE ONLY (the CPU oracle).

Used by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the checker; never by mtr_amd/.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
LIB = os.path.join(ORACLE_DIR, "liboracle_mtr.so")
MAX_PERIOD = 500


class ORecord(C.Structure):
    _fields_ = [("rep_start", C.c_int32), ("rep_end", C.c_int32), ("repeat_len", C.c_int32), ("rep_period", C.c_int32),
                ("num_freq_unit", C.c_int32), ("num_matches", C.c_int32), ("num_mismatches", C.c_int32),
                ("num_insertions", C.c_int32), ("num_deletions", C.c_int32), ("kmer", C.c_int32), ("match_gain", C.c_int32),
                ("mismatch_penalty", C.c_int32), ("indel_penalty", C.c_int32),
                ("unit", C.c_char * (MAX_PERIOD * 2 + 4)), ("unit_score", C.c_int32 * MAX_PERIOD)]


class OStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("dp_calls", "dp_cells", "dp_rows", "dp_max_cells", "revise_dp_calls", "revise_dp_cells",
                                         "kmer_tables", "kmer_lookups", "searches_passing_maxfreq", "ranges_candidate",
                                         "ranges_executed", "records", "di_passes", "di_positions")]


class ODpResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rep_start", "rep_end", "repeat_len", "num_freq_unit", "num_matches",
                                         "num_mismatches", "num_insertions", "num_deletions")]


class OSearchResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("found", "period", "rep_start", "rep_end", "repeat_len", "copies", "mat", "mis", "ins", "del_",
                                         "max_freq", "n_seeds")] + [("seeds", C.c_int32 * 100), ("unit", C.c_char * (MAX_PERIOD + 4))]


class OReviseIn(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rep_start", "rep_end", "repeat_len", "rep_period", "copies", "mat", "mis", "ins", "del_", "kmer", "G", "MM", "D",
                                         "unit_len")] + [("unit", C.c_uint8 * MAX_PERIOD), ("score", C.c_int32 * MAX_PERIOD)]


class OReviseRound(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_start", "in_end", "in_repeat_len", "in_mis", "in_ins", "in_del", "in_len", "threshold", "rev_len", "unchanged",
                                         "candidate", "accepted", "moved")] + [("in_unit", C.c_uint8 * MAX_PERIOD), ("rev_unit", C.c_uint8 * (MAX_PERIOD * 2 + 4))]


class OReviseOut(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rep_start", "rep_end", "repeat_len", "rep_period", "copies", "mat", "mis", "ins", "del_", "kmer", "G", "MM", "D",
                                         "polished_len")] + [("unit", C.c_uint8 * (MAX_PERIOD * 2 + 4)), ("round", OReviseRound * 2)]


RR_FIELDS = ("rep_start", "rep_end", "repeat_len", "rep_period", "copies", "mat", "mis", "ins", "del_", "kmer", "G", "MM", "D")      # rr_t's scalars, in its order

_lib = None
_libc = C.CDLL(None)
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fopen.restype = C.c_void_p
_libc.fclose.argtypes = [C.c_void_p]
_libc.free.argtypes = [C.c_void_p]


def load(build: bool = True):
    global _lib
    if _lib is not None:
        return _lib
    if build:
        subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)
    lib = C.CDLL(LIB)
    lib.mtro_create.argtypes = [C.c_int, C.c_float]
    lib.mtro_create.restype = C.c_void_p
    lib.mtro_destroy.argtypes = [C.c_void_p]
    lib.mtro_set_file_order.argtypes = [C.c_void_p, C.c_int]
    lib.mtro_set_file_order.restype = None
    lib.mtro_process_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.POINTER(ORecord))]
    lib.mtro_process_read.restype = C.c_int
    lib.mtro_get_stats.argtypes = [C.c_void_p]
    lib.mtro_get_stats.restype = C.POINTER(OStats)
    lib.mtro_reset_stats.argtypes = [C.c_void_p]
    lib.mtro_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mtro_ranges.restype = C.c_int
    lib.mtro_ranges_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mtro_ranges_raw.restype = C.c_int
    lib.mtro_wrap_dp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ODpResult)]
    lib.mtro_wrap_dp.restype = C.c_int
    lib.mtro_search_unit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OSearchResult)]
    lib.mtro_search_unit.restype = C.c_int
    lib.mtro_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_char_p]
    lib.mtro_walk.restype = C.c_int
    lib.mtro_revise.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(OReviseIn), C.c_int, C.POINTER(OReviseOut)]
    lib.mtro_revise.restype = C.c_int
    lib.mtro_set_capture.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.mtro_set_capture.restype = None
    lib.mtro_mt_bases.argtypes = [C.c_void_p, C.c_int]
    lib.mtro_chain.argtypes = [C.POINTER(ORecord), C.c_int, C.c_void_p]
    lib.mtro_chain.restype = C.c_int
    _lib = lib
    return lib


class Oracle:
    def __init__(self, manhattan: bool = True, min_match_ratio: float = 0.6):
        self.lib = load()
        self.h = C.c_void_p(self.lib.mtro_create(1 if manhattan else 0, C.c_float(min_match_ratio)))

    def set_file_order(self, on: bool = True):
        """the reference's behaviour on a multi-read file: process() must then be called in file order"""
        self.lib.mtro_set_file_order(self.h, 1 if on else 0)

    def close(self):
        if self.h:
            self.lib.mtro_destroy(self.h)
            self.h = None

    def process(self, codes: np.ndarray):
        """-> list of 15-tuples in the field order of mtr_amd.Record"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        out = C.POINTER(ORecord)()
        n = self.lib.mtro_process_read(self.h, b"", codes.ctypes.data, len(codes), C.byref(out))
        if n < 0:
            raise RuntimeError("oracle failed")
        res = []
        for i in range(n):
            r = out[i]
            per = r.rep_period
            res.append((r.rep_start, r.rep_end, r.repeat_len, per, r.num_freq_unit, r.num_matches, r.num_mismatches,
                        r.num_insertions, r.num_deletions, r.kmer, r.match_gain, r.mismatch_penalty, r.indel_penalty,
                        r.unit.decode(), tuple(r.unit_score[:max(0, min(per, MAX_PERIOD))])))
        if n > 0:
            _libc.free(C.cast(out, C.c_void_p))
        return res

    def stats(self):
        s = self.lib.mtro_get_stats(self.h).contents
        return {n: int(getattr(s, n)) for n, _ in OStats._fields_}

    def ranges(self, codes: np.ndarray):
        """-> list of (start, end, w, di_bits) of the usable ranges after de-duplication"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        L = len(codes)
        di = np.zeros(L, np.float64)
        end = np.zeros(L, np.int32)
        w = np.zeros(L, np.int32)
        self.lib.mtro_ranges(self.h, codes.ctypes.data, L, di.ctypes.data, end.ctypes.data, w.ctypes.data)
        bits = di.view(np.uint64)
        idx = np.nonzero((end > -1) & (end < L) & (di != -1.0))[0]
        return [(int(i), int(end[i]), int(w[i]), int(bits[i])) for i in idx]

    def ranges_raw(self, codes: np.ndarray):
        """-> (ranges as ranges(), raw): raw = int64 array [m, 4] of (start, end, w, k), one row per position that held a DI entry BEFORE
        the de-duplication, in position order - the list the de-duplication chain walks, with the pass (k, w) that recorded each entry"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        L = len(codes)
        di, end, w, raw, kk = np.zeros(L, np.float64), np.zeros(L, np.int32), np.zeros(L, np.int32), np.zeros(L, np.int32), np.zeros(L, np.int32)
        self.lib.mtro_ranges_raw(self.h, codes.ctypes.data, L, di.ctypes.data, end.ctypes.data, w.ctypes.data, raw.ctypes.data, kk.ctypes.data)
        bits = di.view(np.uint64)
        idx = np.nonzero((end > -1) & (end < L) & (di != -1.0))[0]
        alive = np.nonzero(kk > -1)[0]
        return ([(int(i), int(end[i]), int(w[i]), int(bits[i])) for i in idx],
                np.stack([alive, raw[alive], w[alive], kk[alive]], axis=1).astype(np.int64).reshape(-1, 4))

    def search_unit(self, codes: np.ndarray, qs: int, qe: int, k: int):
        """search_De_Bruijn_graph for one (window, k) -> dict: found, the nine fields of capture point G2 (period, rep_start, rep_end,
        repeat_len, copies, mat, mis, ins, del), unit, and what the search started from (max_freq, seeds in the order they are tried)"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        r = OSearchResult()
        rc = self.lib.mtro_search_unit(self.h, codes.ctypes.data, len(codes), qs, qe, k, C.byref(r))
        if rc < 0:
            raise ValueError("mtro_search_unit: bad arguments")
        return {"found": r.found, "period": r.period, "rep_start": r.rep_start, "rep_end": r.rep_end, "repeat_len": r.repeat_len,
                "copies": r.copies, "mat": r.mat, "mis": r.mis, "ins": r.ins, "del": r.del_, "unit": r.unit.decode(),
                "max_freq": r.max_freq, "seeds": list(r.seeds[:r.n_seeds])}

    def walk(self, codes: np.ndarray, qs: int, qe: int, k: int, backward: bool, seed: int):
        """one greedy walk from `seed` on the table of (window, k) -> (period, unit); period 0 = the walk did not close"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        period = C.c_int(0)
        unit = C.create_string_buffer(MAX_PERIOD + 4)
        rc = self.lib.mtro_walk(self.h, codes.ctypes.data, len(codes), qs, qe, k, 1 if backward else 0, seed, C.byref(period), unit)
        if rc < 0:
            raise ValueError("mtro_walk: bad arguments")
        return period.value, unit.value.decode()

    def capture(self, path: str, level: int = 1):
        """the capture lines (G1 .. G4, oracle/ref_capture.c's format) of what follows go to `path`, until end_capture()"""
        self._cap = _libc.fopen(path.encode(), b"w")
        if not self._cap:
            raise OSError(path)
        self.lib.mtro_set_capture(self.h, self._cap, level)

    def end_capture(self):
        self.lib.mtro_set_capture(self.h, None, 0)
        _libc.fclose(self._cap)
        self._cap = None

    def revise(self, codes: np.ndarray, rr, unit, score, polish: bool = True):
        """mtro_revise: revise_representative_unit for one record.  rr: the 13 scalar fields in rr_t's order (rep_start, rep_end, repeat_len, period,
        copies, mat, mis, ins, del, k, G, MM, D), unit: codes 0..3 (len = period), score: its node frequencies; polish=False: the unit is already
        polished.  -> dict: rr (13-tuple), unit (uint8 codes), polished_len, rounds (two dicts: the G3r fields the round was given, threshold,
        rev_len, rev_unit, unchanged, candidate, accepted, moved).  ValueError (the code in it) where the export refuses."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        a, o = OReviseIn(), OReviseOut()
        for n, v in zip(RR_FIELDS, rr):
            setattr(a, n, int(v))
        unit, score = np.asarray(unit, np.uint8), np.asarray(score, np.int32)
        a.unit_len = len(unit)
        if len(unit) <= MAX_PERIOD and len(score) == len(unit):
            C.memmove(a.unit, unit.ctypes.data, len(unit))
            C.memmove(a.score, score.ctypes.data, 4 * len(unit))
        else:
            a.unit_len = -1
        rc = self.lib.mtro_revise(self.h, codes.ctypes.data, len(codes), C.byref(a), 1 if polish else 0, C.byref(o))
        if rc < 0:
            raise ValueError(f"mtro_revise: refused ({rc})")
        rounds = []
        for w in o.round:
            d = {n: int(getattr(w, n)) for n, _ in OReviseRound._fields_[:13]}
            d["in_unit"] = bytes(w.in_unit[:max(0, w.in_len)])
            d["rev_unit"] = bytes(w.rev_unit[:max(0, w.rev_len)])
            rounds.append(d)
        out_rr = tuple(int(getattr(o, n)) for n in RR_FIELDS)
        return {"rr": out_rr, "unit": np.array(o.unit[:max(0, o.rep_period)], np.uint8), "polished_len": int(o.polished_len), "rounds": rounds}

    def wrap_dp(self, codes: np.ndarray, qs: int, qe: int, unit: np.ndarray, G: int, MM: int, D: int):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        unit = np.ascontiguousarray(unit, dtype=np.uint8)
        r = ODpResult()
        rc = self.lib.mtro_wrap_dp(codes.ctypes.data, len(codes), qs, qe, unit.ctypes.data, len(unit), G, MM, D, C.byref(r))
        if rc != 0:
            raise RuntimeError("oracle DP too large")
        return (r.rep_start, r.rep_end, r.repeat_len, r.num_freq_unit, r.num_matches, r.num_mismatches, r.num_insertions, r.num_deletions)


def mt_bases(n: int) -> np.ndarray:
    out = np.zeros(n, np.uint8)
    load().mtro_mt_bases(out.ctypes.data, n)
    return out
