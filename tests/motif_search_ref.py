"""The definition of the known-motif search (include/mtr_hip.h, "known-motif search") in plain Python: the whole matrix, the reference's
loops (wrap_around_DP.c:258-333) with DP row i standing for read base x[i - 1].  Test infrastructure only: tests/test_motif_search_ref.py
holds it to the CPU oracle, the GPU tests use the oracle itself and these read makers."""
from __future__ import annotations

import numpy as np

SCORE_SETS = [(5, 1, 1), (1, 1, 3), (1, 3, 1)]          # the reference's three (match_gain, mismatch_penalty, indel_penalty)
NO_HIT = (0, -1, 0, 0, 0, 0, 0, 0)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def codes_of(motif) -> np.ndarray:
    s = motif.decode() if isinstance(motif, (bytes, bytearray)) else motif
    return np.array([CODE[c] for c in s], np.uint8)


def revcomp(codes: np.ndarray) -> np.ndarray:
    return (3 - np.asarray(codes, np.uint8))[::-1].copy()


def align(x, m, G: int, MM: int, D: int):
    """-> (start, end, repeat_len, copies, matches, mismatches, insertions, deletions, score) of read codes x against motif codes m"""
    x, m = [int(v) for v in x], [int(v) for v in m]
    L, U = len(x), len(m)
    H = [[0] * (U + 1) for _ in range(L + 1)]
    best, bi, bj = 0, 0, 0
    for i in range(1, L + 1):
        row, prev = H[i], H[i - 1]
        for j in range(1, U + 1):
            if x[i - 1] == m[j - 1]:
                v = prev[j - 1] + G
            else:
                v = max(0, prev[j - 1] - MM, prev[j] - D)
                if j > 1:
                    v = max(v, row[j - 1] - D)
            row[j] = v
            if v > best:
                best, bi, bj = v, i, j
        row[0] = row[U]
    if best <= 0:
        return NO_HIT + (0,)
    i, j, cur = bi, bj, best
    mat = mis = ins = dele = 0
    while i > 0 and H[i][j] > 0:
        eq = x[i - 1] == m[j - 1]
        if cur == H[i - 1][j - 1] + G and eq:
            cur -= G; i -= 1; j -= 1; mat += 1
        elif cur == H[i - 1][j - 1] - MM and not eq:
            cur += MM; i -= 1; j -= 1; mis += 1
        elif cur == H[i][j - 1] - D:
            cur += D; j -= 1; dele += 1
        elif cur == H[i - 1][j] - D:
            cur += D; i -= 1; ins += 1
        else:
            assert cur == 0, "the matrix is inconsistent"
            break
        if j == 0:
            j = U
    return (i, bi - 1, bi - i, (mat + mis + dele) // U, mat, mis, ins, dele, best)


def search(x, motif_codes, G: int, MM: int, D: int, both_strands: bool = True, one=align):
    """-> (the nine values, strand): the better strand, the forward motif on a tie.  one: the aligner (align, or the oracle's)"""
    fwd = one(x, motif_codes, G, MM, D)
    if not both_strands:
        return fwd, 0
    rev = one(x, revcomp(motif_codes), G, MM, D)
    return (rev, 1) if rev[8] > fwd[8] else (fwd, 0)


def oracle_align(orc):
    """the same nine values from the CPU oracle: wrap_around_DP_sub on the read shifted by one base, rep_start and rep_end lowered by one,
    the score by the identity (include/mtr_hip.h)"""
    def one(x, m, G, MM, D):
        x = np.asarray(x, np.uint8)
        w = orc.wrap_dp(np.concatenate([np.zeros(1, np.uint8), x]), 0, len(x) - 1, np.asarray(m, np.uint8), G, MM, D)
        f = (w[0] - 1, w[1] - 1) + tuple(w[2:])
        return f + (G * f[4] - MM * f[5] - D * (f[6] + f[7]),)
    return one


# ---- reads ------------------------------------------------------------------------------------------------------------
KINDS = ("random", "tandem", "two_runs", "no_hit")


def make_read(rng, kind: str, L: int, m: np.ndarray) -> np.ndarray:
    """random: uniform bases.  tandem: copies of m starting mid-unit, about one base in eleven changed, dropped or inserted.  two_runs: a clean
    run, junk, the same run again (the first must win).  no_hit: a base m does not hold (uniform bases when m holds all four)."""
    U = len(m)
    absent = [c for c in range(4) if c not in set(int(v) for v in m)]
    if kind == "random":
        return rng.randint(0, 4, size=L).astype(np.uint8)
    if kind == "tandem":
        out, ph = [], U // 2
        while len(out) < L:
            e = rng.randint(0, 33)
            if e == 0:
                out.append((int(m[ph % U]) + 1 + rng.randint(0, 3)) & 3); ph += 1
            elif e == 1:
                ph += 1
            elif e == 2:
                out.append(rng.randint(0, 4))
            else:
                out.append(int(m[ph % U])); ph += 1
        return np.array(out[:L], np.uint8)
    if kind == "two_runs":
        run = max(1, L // 3)
        x = np.array([m[i % U] for i in range(L)], np.uint8)
        for i in range(run, L - run):
            x[i] = absent[-1] if absent else (int(m[i % U]) + 2) & 3
        for i in range(max(run, L - run), L):
            x[i] = m[(i - (L - run)) % U]
        return x
    if kind == "no_hit":
        return np.full(L, absent[-1], np.uint8) if absent else rng.randint(0, 4, size=L).astype(np.uint8)
    raise ValueError(kind)
