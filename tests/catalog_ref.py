"""The definition of the catalogue genotype (include/mtr_hip.h, "catalogue genotype") in plain Python: the seeds of a pattern, the candidates by
set lookup on a read's q-mers, and then tests/flank_ref.py's hits and pairing on the candidates alone.  Test infrastructure only:
tests/test_catalog_ref.py holds it to hand-worked cases, the GPU tests take its candidate counts as truth (their rows' truth is the dense call)."""
from __future__ import annotations

import numpy as np

from tests import flank_ref as fref
from tests import motif_search_ref as ref


def seeds(p, K: int, q: int):
    """the K + 1 disjoint seeds of pattern p, as tuples"""
    assert len(p) >= (K + 1) * q, (len(p), K, q)
    return [tuple(int(c) for c in p[i * q:(i + 1) * q]) for i in range(K + 1)]


def slots(locus):
    """the four flank patterns of a locus: A, B, rc A, rc B"""
    A, _, B = locus
    return [np.asarray(A, np.uint8), np.asarray(B, np.uint8), ref.revcomp(np.asarray(A, np.uint8)), ref.revcomp(np.asarray(B, np.uint8))]


def qmers(read, q: int):
    r = [int(c) for c in read]
    return {tuple(r[p:p + q]) for p in range(len(r) - q + 1)}


def seeded(read_qmers, p, K: int, q: int):
    """the indices of the seeds of p that the read holds"""
    return [i for i, s in enumerate(seeds(p, K, q)) if s in read_qmers]


def seed_index(loci, K: int, q: int):
    """seed -> the set of (locus, slot) it belongs to"""
    index = {}
    for l, locus in enumerate(loci):
        for slot, p in enumerate(slots(locus)):
            for s in seeds(p, K, q):
                index.setdefault(s, set()).add((l, slot))
    return index


def read_hits(reads, loci, K: int, q: int):
    """per read the set of (locus, slot) of which it holds a seed"""
    index = seed_index(loci, K, q)
    out = []
    for r in reads:
        got = set()
        for s in qmers(r, q):
            got |= index.get(s, set())
        out.append(got)
    return out


def candidates(reads, loci, K: int, q: int):
    """the (read, locus, orientation) with a seed of both of the orientation's patterns in the read, sorted"""
    out = []
    for r, got in enumerate(read_hits(reads, loci, K, q)):
        out += [(r, l, slot >> 1) for (l, slot) in got if slot & 1 == 0 and (l, slot + 1) in got]
    return sorted(out)


def genotype(reads, loci, K: int, q: int, G: int = 1, MM: int = 1, D: int = 1, one=ref.align):
    """-> (rows, candidates): rows = the sorted list of (read, locus, orientation, (left, right), (lo, hi), fields[8], score, ratio) of the spanning
    pairs, a non-candidate orientation counted as invalid"""
    cands = candidates(reads, loci, K, q)
    memo = {}

    def hit(r, p):
        key = (r, bytes(bytearray(int(c) for c in p)))
        if key not in memo:
            memo[key] = tuple(int(c[0]) for c in fref.hits([reads[r]], p))
        return memo[key]

    far = (K + 1, 0, 0)
    rows = []
    for r, l in sorted({(r, l) for r, l, _ in cands}):
        four = [hit(r, p) if (r, l, slot >> 1) in set(cands) else far for slot, p in enumerate(slots(loci[l]))]
        sp, o, dl, dr, lo, hi = fref.pair(*four, K)
        if not sp:
            continue
        fields, score, ratio = (0,) * 8, 0, np.float32(0)
        if hi > lo:
            M = np.asarray(loci[l][1], np.uint8)
            h = one(np.asarray(reads[r][lo:hi], np.uint8), ref.revcomp(M) if o else M, G, MM, D)
            fields, score = (h[0] + lo, h[1] + lo) + tuple(int(v) for v in h[2:8]), int(h[8])
            ratio = np.float32(h[4]) / np.float32(h[2]) if h[2] > 0 else np.float32(0)
        rows.append((r, l, o, (dl, dr), (lo, hi), tuple(int(v) for v in fields), score, ratio))
    return rows, cands
