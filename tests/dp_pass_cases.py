"""Seeded cases for the forward passes of the wrap-around DP: the smallest shapes at which the passes can go wrong (test infrastructure only).

A case is one DP: a read, a window (qs, qe) of it, a unit, a parameter set.  Row i of the DP stands for base qs + i of the read, so every window keeps
qe <= L - 2 (the oracle's wrap_dp reads codes[qe + 1]); qe = L - 2, the last row on
the read's last base, occurs throughout.  A Batch collects the reads of the cases of one test; its groups are what
Engine.test_wrap_dp_pass takes, its tasks what Engine.test_wrap_dp takes.  tests/test_dp_pass_cases_ref.py shows from the oracle alone that
the cases are not degenerate; tests/test_gpu_dp_passes.py runs them on the kernels.
"""
from __future__ import annotations

import numpy as np

SETS2 = ((1, 1, 3), (1, 3, 1))                           # wrap_around_DP's two calls, in that order
SETS3 = ((1, 1, 3), (1, 3, 1), (5, 1, 1))                # + the vote DP of the revisions
U16 = (2, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128)      # either side of every columns-per-lane border of the 16-lane passes
U64 = U16 + (129, 192, 193, 256, 257, 499)               # the passes with one DP per wavefront as well
ROWS_FIXED = (1, 2, 239, 240, 241, 1007, 1008, 1009)     # + U - 1, U, U + 1; 240 / 1008: the staged chunk of a 16-lane / 64-lane pass
QS_MOD = (0, 1, 15)
KINDS = ("perfect", "noisy", "random", "absent", "two_runs", "homopolymer", "ac")
# 16-bit limits (scores times DPQ_SCALE = 4 in the 16-lane passes, times one in the others); mirrors of the macros of mtr_amd/csrc
DPQ_LIMIT = 65000


def dpq_max_rows(U: int, G: int, D: int, scale: int = 4) -> int:
    """the largest rows with scale * (rows G + D (U + 2)) < 65000: DPQ_FITS (scale 4), DP2C_FITS and DPQ_FITS_SC(1, ...) (scale 1)"""
    return ((DPQ_LIMIT - 1) // scale - D * (U + 2)) // G


class Case:
    __slots__ = ("read", "qs", "qe", "unit", "G", "MM", "D", "kind", "tag")

    def __init__(self, read, qs, qe, unit, params=(1, 1, 3), kind="", tag=""):
        self.read, self.qs, self.qe, self.unit = read, int(qs), int(qe), np.asarray(unit, np.uint8)
        self.G, self.MM, self.D = params
        self.kind, self.tag = kind, tag

    @property
    def U(self):
        return len(self.unit)

    @property
    def rows(self):
        return self.qe - self.qs + 1

    def with_params(self, params):
        return Case(self.read, self.qs, self.qe, self.unit, params, self.kind, self.tag)

    def __repr__(self):
        return f"<{self.tag or self.kind} U={self.U} rows={self.rows} qs={self.qs} set=({self.G},{self.MM},{self.D})>"


# ---- content -------------------------------------------------------------------------------------------------------------------------
def make_unit(rng, U: int, kind: str) -> np.ndarray:
    if kind == "homopolymer":
        return np.zeros(U, np.uint8)
    if kind == "ac":
        return np.array([0, 1] * (U // 2) + [0] * (U & 1), np.uint8)
    letters = 3 if kind in ("absent", "two_runs") else 4            # these kinds need a base the unit lacks
    m = rng.randint(0, letters, size=U).astype(np.uint8)
    if U >= letters:
        m[rng.permutation(U)[:letters]] = np.arange(letters, dtype=np.uint8)     # every letter at least once
    return m


def make_window(rng, kind: str, rows: int, m: np.ndarray) -> np.ndarray:
    """the bases of the window's rows.  perfect: copies of m starting mid-unit.  noisy: the same with about 12 % of the bases changed, dropped or
    inserted.  random: uniform.  absent: a base m lacks.  two_runs: a clean run, junk (that base), the same run again.  homopolymer / ac: m repeated."""
    U = len(m)
    if kind in ("perfect", "homopolymer", "ac"):
        ph = U // 2 if kind == "perfect" else 0
        return np.array([m[(ph + i) % U] for i in range(rows)], np.uint8)
    if kind == "random":
        return rng.randint(0, 4, size=rows).astype(np.uint8)
    if kind == "absent":
        return np.full(rows, 3, np.uint8)
    if kind == "noisy":
        out, ph = [], U // 2
        while len(out) < rows:
            e = rng.randint(0, 25)
            if e == 0:
                out.append((int(m[ph % U]) + 1 + rng.randint(0, 3)) & 3); ph += 1
            elif e == 1:
                ph += 1
            elif e == 2:
                out.append(rng.randint(0, 4))
            else:
                out.append(int(m[ph % U])); ph += 1
        return np.array(out[:rows], np.uint8)
    if kind == "two_runs":
        run = max(1, rows // 3)
        x = np.full(rows, 3, np.uint8)
        for i in range(min(run, rows)):
            x[i] = m[i % U]
        for i in range(max(run, rows - run), rows):
            x[i] = m[(i - (rows - run)) % U]
        return x
    raise ValueError(kind)


def make_case(rng, U: int, rows: int, qs: int, kind: str, params=(1, 1, 3), tail: int = 1, tag: str = "") -> Case:
    """a read of qs + 1 bases in front of the window (random; base 0 .. qs), the window's rows, `tail` >= 0 bases behind it (0: the last row is the
    read's last base, qe = L - 2)"""
    m = make_unit(rng, U, kind)
    read = np.concatenate([rng.randint(0, 4, size=qs + 1).astype(np.uint8), make_window(rng, kind, rows, m), rng.randint(0, 4, size=tail).astype(np.uint8)])
    return Case(read, qs, qs + rows - 1, m, params, kind, tag)


def limit_case(U: int, rows: int, params, qs: int = 5, tag: str = "limit") -> Case:
    """a perfect repeat of `rows` rows starting mid-unit: the score reaches rows x G"""
    rng = np.random.RandomState(1000 * U + qs)
    return make_case(rng, U, rows, qs, "perfect", params, 1, tag)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
def rows_of(U: int):
    return sorted(set(r for r in ROWS_FIXED + (U - 1, U, U + 1) if r >= 1))


def grid(units=U16, seed: int = 1, params=(1, 1, 3), max_rows: int = 1 << 30):
    """every unit length x every row count; content kind and placement cycle through theirs, so each appears with every unit length and row count over
    a few neighbours; the cycle starts at the seed, so the grids of different passes give one shape different kinds and placements.  One case in
    four ends with its read (no base behind the window).  Reads stay under 1 100 bases."""
    rng = np.random.RandomState(seed)
    out, k = [], seed
    for U in units:
        for rows in rows_of(U):
            if rows > max_rows:
                continue
            kind = KINDS[k % len(KINDS)]
            if kind == "ac" and U & 1:
                kind = "perfect"
            qs = 16 * rng.randint(0, 3) + QS_MOD[(k // len(KINDS)) % 3]
            out.append(make_case(rng, U, rows, qs, kind, params, rng.randint(0, 4), "grid"))
            k += 1
    return out


def small_grid(seed: int = 2):
    """rows <= 41 and U <= 33, every kind and placement: small enough for the plain-Python definition (tests/motif_search_ref.align)"""
    rng = np.random.RandomState(seed)
    out = []
    for U in (2, 16, 17, 32, 33):
        for rows in sorted(set((1, 2, U - 1, U, U + 1, 41))):
            if rows < 1 or rows > 41:
                continue
            for kind in KINDS:
                if kind == "ac" and U & 1:
                    continue
                for mod in QS_MOD:
                    for params in SETS3:
                        out.append(make_case(rng, U, rows, mod, kind, params, 1, "small"))
    return out


# ---- a batch: the reads of a test's cases, and the task tuples of the engine -----------------------------------------------------------------
class Batch:
    def __init__(self):
        self.reads, self.cases, self.read_of = [], [], []

    def add(self, case: Case) -> int:
        for i, r in enumerate(self.reads):
            if r is case.read:
                break
        else:
            i = len(self.reads)
            self.reads.append(case.read)
        self.cases.append(case)
        self.read_of.append(i)
        return len(self.cases) - 1

    def task(self, k: int):
        c = self.cases[k]
        return (self.read_of[k], c.qs, c.qe, c.unit, c.G, c.MM, c.D)

    def groups(self, index_groups):
        return [[self.task(k) for k in g] for g in index_groups]


_want = {}


def oracle_want(orc, case: Case, params=None):
    """Oracle.wrap_dp of the case (with another parameter set, if given), computed once per process"""
    G, MM, D = params or (case.G, case.MM, case.D)
    key = (id(case.read), case.qs, case.qe, case.unit.tobytes(), G, MM, D)
    if key not in _want:
        _want[key] = (case.read, tuple(int(v) for v in orc.wrap_dp(case.read, case.qs, case.qe, case.unit, G, MM, D)))      # (the read is kept: its id stays its own)
    return _want[key][1]


# ---- the passes' cases -------------------------------------------------------------------------------------------------------------------
def chunk(items, n):
    return [items[i:i + n] for i in range(0, len(items), n)]


def placement_cases(rng, U: int, kind: str = "noisy"):
    """(first, last): a window at the start of its read (to be the batch's first read) and one whose last row is the last base of its read (the last read)"""
    first = make_case(rng, U, 3 * U + 5, 0, kind, tag="start of the first read")
    last = make_case(rng, U, 3 * U + 7, 15, "perfect", tail=0, tag="last base of the last read")       # a perfect repeat: its last row must count
    assert first.qs == 0 and last.qe + 1 == len(last.read) - 1
    return first, last


def wave2p_limits():
    out = []
    for U in (2, 64, 65, 128, 129, 256):
        long = limit_case(U, 64001, (1, 1, 3), tag="WAVE2P limit")
        out.append(Case(long.read, long.qs, long.qe - 1, long.unit, (1, 1, 3), "perfect", "WAVE2P limit 64000"))
        out.append(long)
    for U in (17, 128):                                     # one row more than QUAD2P takes
        out.append(limit_case(U, 16243 - 3 * U + 1, (1, 1, 3), tag="QUAD2P limit + 1"))
    return out


def quad2p_limits():
    return [limit_case(U, 16243 - 3 * U, (1, 1, 3), tag="QUAD2P limit") for U in (17, 128)]


def one_param_limits():
    """(U, the limit case) for each of the three sets and U in 2, 17, 128"""
    return [limit_case(U, dpq_max_rows(U, G, D), (G, MM, D), tag="1p limit") for U in (2, 17, 128) for (G, MM, D) in SETS3]


def entry_limits():
    """the existing entry: the largest rows of its two 16-bit passes (dp_forward_2c: units 65 .. 128; one DP on 64 lanes: 129 .. 256) and one row more"""
    out = []
    for U in (65, 128, 129, 256):
        for (G, MM, D) in SETS3:
            rows = dpq_max_rows(U, G, D, 1)
            long = limit_case(U, rows + 1, (G, MM, D), tag="entry limit + 1")
            out.append(Case(long.read, long.qs, long.qe - 1, long.unit, (G, MM, D), "perfect", "entry limit"))
            out.append(long)
    return out
