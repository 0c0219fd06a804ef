"""The definition of the partial genotype (include/mtr_hip.h, "partial genotype") in plain Python / numpy: the flank hits of tests/flank_ref.py,
the genotype's pairing rule, the choice of slot, and the anchored extension as a whole matrix of (H, C, T) cells.  Test infrastructure only:
tests/test_partial_ref.py holds it to hand-worked extensions, the GPU tests take it as truth."""
from __future__ import annotations

import numpy as np

from tests import flank_ref as fref
from tests import motif_search_ref as ref

SUB_LEFT_UP = (0, 1, 2)          # the definition's predecessor priority: diagonal, deletion, insertion
UP_LEFT_SUB = (2, 1, 0)          # reversed: what test_partial_ref.py uses to show that the inputs depend on the rule


def extend(y, m, G: int = 1, MM: int = 1, D: int = 1, priority=SUB_LEFT_UP):
    """the extension of y against m -> (ext_len, motif_bases, matches, score); zeros without a positive cell"""
    n, U = len(y), len(m)
    prev = [(0, 0, 0)] * (U + 1)                                  # (H, C, T) of row i - 1, column 0 = column U
    best = (0, 0, 0, 0)
    for i in range(1, n + 1):
        cur = [None] * (U + 1)
        for j in range(1, U + 1):
            dH, dC, dT = prev[j - 1] if j > 1 else prev[U]
            match = int(y[i - 1]) == int(m[j - 1])
            cand = {0: (dH + (G if match else -MM), dC + 1, dT + (1 if match else 0)), 2: (prev[j][0] - D, prev[j][1], prev[j][2])}
            if j > 1:
                cand[1] = (cur[j - 1][0] - D, cur[j - 1][1] + 1, cur[j - 1][2])
            h = max(c[0] for c in cand.values())
            cur[j] = next(cand[k] for k in priority if k in cand and cand[k][0] == h)
            if h > best[3]:
                best = (i, cur[j][1], cur[j][2], h)
        cur[0] = cur[U]
        prev = cur
    return best


def choose(four, K: int, L: int):
    """the four single-strand hits (dist, start, end) of A, B, rc A, rc B -> None (spanning, or no flank within K) or (slot, dist, lo, hi)"""
    if fref.pair(*four, K)[0]:
        return None
    near = [(f[0], s) for s, f in enumerate(four) if f[0] <= K]
    if not near:
        return None
    dist, s = min(near)
    lo, hi = (four[s][2], L) if s in (0, 3) else (0, four[s][1])
    return s, int(dist), int(lo), int(hi)


def oriented(x, M, slot: int, lo: int, hi: int):
    """the row's y and m"""
    Mo = ref.revcomp(M) if slot >> 1 else np.asarray(M, np.uint8)
    back = slot in (1, 2)
    w = np.asarray(x[lo:hi], np.uint8)
    return (w[::-1], Mo[::-1]) if back else (w, Mo)


def genotype_partial(reads, loci, K: int, G: int = 1, MM: int = 1, D: int = 1, max_tail: int = 10, priority=SUB_LEFT_UP):
    """-> PartialGenotypes' columns as numpy for loci = [(left, motif, right)] of code arrays"""
    n, m = len(reads), len(loci)
    partial, slot, is_open = np.zeros((n, m), np.uint8), np.zeros((n, m), np.uint8), np.zeros((n, m), np.uint8)
    fdist, window, ext = np.zeros((n, m), np.int32), np.zeros((n, m, 2), np.int32), np.zeros((n, m, 6), np.int32)
    ratio = np.zeros((n, m), np.float32)
    for k, (A, M, B) in enumerate(loci):
        four = [fref.hits(reads, q) for q in (A, B, ref.revcomp(A), ref.revcomp(B))]
        for r in range(n):
            c = choose([tuple(int(v[r]) for v in f) for f in four], K, len(reads[r]))
            if c is None:
                continue
            s, dist, lo, hi = c
            y, mo = oriented(reads[r], M, s, lo, hi)
            bi, C, T, H = extend(y, mo, G, MM, D, priority)
            partial[r, k], slot[r, k], fdist[r, k], window[r, k] = 1, s, dist, (lo, hi)
            ext[r, k] = (bi, C, C // len(M), T, H, hi - lo - bi)
            ratio[r, k] = np.float32(T) / np.float32(bi) if bi > 0 else np.float32(0)
            is_open[r, k] = 1 if hi - lo - bi <= max_tail else 0
    return partial, slot, fdist, window, ext, ratio, is_open
