"""The definition of the partial genotype at catalogue scale (include/mtr_hip.h, "partial genotype at catalogue scale") in plain Python: the
candidates by tests/catalog_ref.py's set lookup on a read's q-mers (a seed of ANY of the four slots), tests/flank_ref.py's hits on the seeded
slots alone - an unseeded slot counts as beyond K -, and tests/partial_ref.py's choice and extension.  Test infrastructure only:
tests/test_partial_catalog_ref.py holds it to the dense reference, the GPU tests take its candidate counts as truth (their rows' truth is the
dense call)."""
from __future__ import annotations

import numpy as np

from tests import catalog_ref as cref
from tests import flank_ref as fref
from tests import partial_ref as pref


def candidates(reads, loci, K: int, q: int):
    """-> the sorted list of (read, locus, mask): mask bit s set where the read holds a seed of slot s of the locus"""
    out = []
    for r, got in enumerate(cref.read_hits(reads, loci, K, q)):
        masks = {}
        for l, slot in got:
            masks[l] = masks.get(l, 0) | 1 << slot
        out += [(r, l, mask) for l, mask in masks.items()]
    return sorted(out)


def seeded_hits(reads, loci, cands):
    """(read, locus, slot) -> (dist, start, end), the flank search's own hit over the whole read, for the seeded slots of the candidates and for
    no other: a pattern meets only the reads that hold one of its seeds (all of them in one call of flank_ref.hits)"""
    who = {}
    for r, l, mask in cands:
        for s in range(4):
            if mask >> s & 1:
                who.setdefault((l, s), []).append(r)
    out = {}
    for (l, s), rs in who.items():
        f = fref.hits([reads[r] for r in rs], cref.slots(loci[l])[s])
        for i, r in enumerate(rs):
            out[(r, l, s)] = tuple(int(c[i]) for c in f)
    return out


def four_hits(found, r: int, l: int, mask: int, K: int):
    """the four (dist, start, end) of a candidate: found's hit for a seeded slot, beyond K for the others"""
    return [found[(r, l, s)] if mask >> s & 1 else (K + 1, 0, 0) for s in range(4)]


def genotype_partial_catalog(reads, loci, K: int, q: int, G: int = 1, MM: int = 1, D: int = 1, max_tail: int = 10, priority=pref.SUB_LEFT_UP):
    """-> (rows, candidates): rows = the sorted list of (read, locus, slot, dist, (lo, hi), ext[6], ratio, open) of the partial pairs"""
    cands = candidates(reads, loci, K, q)
    found = seeded_hits(reads, loci, cands)
    rows = []
    for r, l, mask in cands:
        c = pref.choose(four_hits(found, r, l, mask, K), K, len(reads[r]))
        if c is None:
            continue
        s, dist, lo, hi = c
        M = loci[l][1]
        y, mo = pref.oriented(reads[r], M, s, lo, hi)
        bi, C, T, H = pref.extend(y, mo, G, MM, D, priority)
        ratio = np.float32(T) / np.float32(bi) if bi > 0 else np.float32(0)
        rows.append((r, l, s, dist, (lo, hi), (bi, C, C // len(M), T, H, hi - lo - bi), ratio, 1 if hi - lo - bi <= max_tail else 0))
    return rows, cands


def dense_rows(cols):
    """the partial rows of partial_ref.genotype_partial's columns, in the layout of genotype_partial_catalog's rows"""
    partial, slot, fdist, window, ext, ratio, is_open = cols
    return [(int(r), int(k), int(slot[r, k]), int(fdist[r, k]), tuple(int(v) for v in window[r, k]), tuple(int(v) for v in ext[r, k]), ratio[r, k], int(is_open[r, k]))
            for r, k in zip(*np.nonzero(partial))]
