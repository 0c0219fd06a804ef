"""The definitions of the flank search and of the locus genotyping (include/mtr_hip.h, "flank search", "locus genotyping") in plain
Python / numpy: the whole edit-distance matrix column by column - no bit vectors - and the pairing rules over its hits.  Test infrastructure
only: tests/test_flank_ref.py holds it to brute force (ed() of every substring), the GPU tests take it as truth."""
from __future__ import annotations

import numpy as np

from tests import motif_search_ref as ref

LETTERS = "ACGT"


def text(codes) -> str:
    return "".join(LETTERS[int(c)] for c in codes)


def ed(a, b) -> int:
    """unit-cost edit distance, the whole matrix"""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, cb in enumerate(b, 1):
            cur[j] = min(prev[j - 1] + (int(ca) != int(cb)), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def brute(p, x):
    """(dist, start, end) from the definition's words alone: ed() of every substring.  Small cases only."""
    L = len(x)
    d = [min(ed(p, x[s:e]) for s in range(e + 1)) for e in range(L + 1)]
    dist = min(d)
    end = d.index(dist)
    start = max(s for s in range(end + 1) if ed(p, x[s:end]) == dist)
    return dist, start, end


def _padded(reads):
    n, lmax = len(reads), max([len(r) for r in reads] + [1])
    X = np.full((n, lmax), 4, np.int64)                      # 4: a base no pattern holds
    for i, r in enumerate(reads):
        X[i, :len(r)] = r
    return X, np.array([len(r) for r in reads], np.int64)


def _column(col, neq, row0):
    """the next column of D(i, e) = min(D(i-1, e-1) + neq, D(i-1, e) + 1, D(i, e-1) + 1) for every read at once; row0: its D(0, .)"""
    m = neq.shape[1]
    u = np.concatenate([row0[:, None], np.minimum(col[:, :-1] + neq, col[:, 1:] + 1)], axis=1)
    ramp = np.arange(m + 1)
    return np.minimum.accumulate(u - ramp, axis=1) + ramp    # the vertical term: min over k <= i of u[k] + (i - k)


def hits(reads, p):
    """the single-strand hit F(p) of every read: (dist, start, end), int64 [n] each"""
    p = np.asarray(p, np.int64)
    m, n = len(p), len(reads)
    X, lens = _padded(reads)
    col = np.tile(np.arange(m + 1), (n, 1))
    dist, end = np.full(n, m, np.int64), np.zeros(n, np.int64)
    zero = np.zeros(n, np.int64)
    for e in range(int(lens.max()) if n else 0):
        new = _column(col, (X[:, e:e + 1] != p[None, :]).astype(np.int64), zero)
        live = e < lens
        col = np.where(live[:, None], new, col)
        better = live & (new[:, m] < dist)
        dist, end = np.where(better, new[:, m], dist), np.where(better, e + 1, end)
    # start: the reversed pattern against x[end - 1], x[end - 2], ..: column j's last cell is ed(p, x[end - j .. end)); the first j that gives dist
    rp = p[::-1]
    col = np.tile(np.arange(m + 1), (n, 1))
    start = np.where(dist == m, end, -1)
    for j in range(1, int(end.max()) + 1 if n else 0):
        at = end - j
        base = np.where(at >= 0, X[np.arange(n), np.maximum(at, 0)], 4)
        col = _column(col, (base[:, None] != rp[None, :]).astype(np.int64), np.full(n, j, np.int64))
        found = (start < 0) & (at >= 0) & (col[:, m] == dist)
        start = np.where(found, at, start)
        if (start >= 0).all():
            break
    assert (start >= 0).all() and ((end - start) <= m + dist).all()
    return dist, start, end


def search(reads, patterns, both_strands: bool = True):
    """-> FlankHits' columns as numpy: dist, start, end (int32 [n, m]) and strand (uint8 [n, m]); patterns: code arrays"""
    n, m = len(reads), len(patterns)
    out = [np.zeros((n, m), np.int32) for _ in range(3)] + [np.zeros((n, m), np.uint8)]
    for k, p in enumerate(patterns):
        f = hits(reads, p)
        strand = np.zeros(n, bool)
        if both_strands:
            r = hits(reads, ref.revcomp(p))
            strand = r[0] < f[0]
            f = tuple(np.where(strand, b, a) for a, b in zip(f, r))
        for c in range(3):
            out[c][:, k] = f[c]
        out[3][:, k] = strand
    return tuple(out)


def pair(a, b, ra, rb, K: int):
    """the pairing rules on the four single-strand hits (dist, start, end) of A, B, rc A, rc B -> (spanning, orientation, left, right, lo, hi)"""
    v0 = a[0] <= K and b[0] <= K and a[2] <= b[1]
    v1 = ra[0] <= K and rb[0] <= K and rb[2] <= ra[1]
    if not (v0 or v1):
        return (0, 0, 0, 0, 0, 0)
    o = 1 if (v1 and not v0) or (v0 and v1 and ra[0] + rb[0] < a[0] + b[0]) else 0
    return (1, 1, int(ra[0]), int(rb[0]), int(rb[2]), int(ra[1])) if o else (1, 0, int(a[0]), int(b[0]), int(a[2]), int(b[1]))


def genotype(reads, loci, K: int, G: int = 1, MM: int = 1, D: int = 1, one=ref.align):
    """-> Genotypes' columns as numpy for loci = [(left, motif, right)] of code arrays; one: the aligner (ref.align, or the oracle's).
    Also the list of (read, locus, kind) of the pairs that do not span: 'left', 'right' (that flank alone is beyond K in both orientations' best),
    'order' (both flanks within K in an orientation, in the wrong order)."""
    n, m = len(reads), len(loci)
    spanning, orientation = np.zeros((n, m), np.uint8), np.zeros((n, m), np.uint8)
    fdist, window, fields = np.zeros((n, m, 2), np.int32), np.zeros((n, m, 2), np.int32), np.zeros((n, m, 8), np.int32)
    score, ratio = np.zeros((n, m), np.int32), np.zeros((n, m), np.float32)
    why = []
    for k, (A, M, B) in enumerate(loci):
        four = [hits(reads, q) for q in (A, B, ref.revcomp(A), ref.revcomp(B))]
        for r in range(n):
            a, b, ra, rb = [tuple(int(c[r]) for c in f) for f in four]
            sp, o, dl, dr, lo, hi = pair(a, b, ra, rb, K)
            spanning[r, k], orientation[r, k], fdist[r, k], window[r, k] = sp, o, (dl, dr), (lo, hi)
            if not sp:
                near0, near1 = a[0] <= K and b[0] <= K, ra[0] <= K and rb[0] <= K
                why.append((r, k, "order" if near0 or near1 else "left" if min(a[0], ra[0]) > K and min(b[0], rb[0]) <= K else
                            "right" if min(b[0], rb[0]) > K and min(a[0], ra[0]) <= K else "both"))
                continue
            if hi > lo:
                h = one(np.asarray(reads[r][lo:hi], np.uint8), ref.revcomp(M) if o else np.asarray(M, np.uint8), G, MM, D)
                fields[r, k] = (h[0] + lo, h[1] + lo) + tuple(h[2:8])
                score[r, k] = h[8]
                ratio[r, k] = np.float32(h[4]) / np.float32(h[2]) if h[2] > 0 else np.float32(0)
    return (spanning, orientation, fdist, window, fields, score, ratio), why
