"""The seeded inputs of the partial genotype's tests (tests/test_partial_ref.py on the CPU, tests/test_gpu_partial.py on the GPU) and their
reference columns, computed once per (K, scores) by tests/partial_ref.py and shared.

LOCI    ten loci, motifs of 1, 2, 3, 4, 5, 8, 9, 16, 17 and 32 bases (every bucket at both of its edges), flanks of 20 .. 24 bases.
GRID    per locus and slot sixteen reads: read i's window begins (forward slots) or ends (backward slots, whose windows begin at base 0) at
        residue i mod 16, and a forward window ends - with its read - at residue 5 i + 3 mod 16.  Every other read - the odd ones of an even
        locus, the even ones of an odd locus, so that either K sees every residue - carries one or two edits in its flank (found with K = 3,
        lost with K = 0) and noise in the repeat; reads 4 .. 7 and 12 .. 15 close the repeat with 15 .. 30 other bases; the repeat starts at
        phase i of its motif; windows are 30 .. 110 bases.
EXTRA   the cases a grid does not hold: ties of dist between slots, empty windows, windows shorter than the motif, windows without a positive
        cell, spanning reads, a read without any flank, one base."""
from __future__ import annotations

import numpy as np

from tests import flank_ref as fref
from tests import motif_search_ref as ref
from tests import partial_ref as pref

US = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
SCORES = [(1, 1, 1), (2, 3, 2), (5, 4, 7)]
KS = (0, 3)
MAX_TAIL = 10


def edited(rng, p, edits):
    q = [int(v) for v in p]
    for _ in range(edits):
        at, what = int(rng.randint(0, len(q))), int(rng.randint(0, 3))
        if what == 0:
            q[at] = (q[at] + 1 + int(rng.randint(0, 3))) & 3
        elif what == 1 and len(q) > 1:
            del q[at]
        else:
            q.insert(at, int(rng.randint(0, 4)))
    return np.array(q, np.uint8)


def cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in parts]).astype(np.uint8)


def _loci():
    rng = np.random.RandomState(71)
    out = []
    for k, U in enumerate(US):
        M = rng.randint(0, 4, size=U).astype(np.uint8)
        while U > 1 and len(set(M.tolist())) == 1:
            M = rng.randint(0, 4, size=U).astype(np.uint8)
        out.append((rng.randint(0, 4, size=20 + k % 5).astype(np.uint8), M, rng.randint(0, 4, size=24 - k % 5).astype(np.uint8)))
    return out


LOCI = _loci()
TEXTS = [tuple(fref.text(s) for s in locus) for locus in LOCI]


def repeat(M, phase, length):
    U = len(M)
    return np.tile(M, (phase + length) // U + 2)[phase % U:phase % U + length]


def grid_read(rng, locus, slot, i, noisy):
    """read i of (locus, slot): see the module's text"""
    A, M, B = locus
    closed = (i // 4) % 2
    flank = (A, B, ref.revcomp(A), ref.revcomp(B))[slot]
    mo = ref.revcomp(M) if slot >> 1 else M
    flank = edited(rng, flank, noisy * (1 + (i // 2) % 2))
    closing = rng.randint(0, 4, size=int(rng.randint(15, 31))).astype(np.uint8) if closed else np.zeros(0, np.uint8)
    junk = rng.randint(0, 4, size=int(rng.randint(0, 16))).astype(np.uint8)
    wl = 30 + 4 * i + int(rng.randint(0, 12))
    if slot in (0, 3):                                       # forward: junk + flank + repeat + closing
        while (len(junk) + len(flank)) % 16 != i:
            junk = cat(junk, rng.randint(0, 4, size=1))
        while (len(junk) + len(flank) + wl + len(closing)) % 16 != (5 * i + 3) % 16:
            wl += 1
        rep = repeat(mo, i, wl)
        rep = edited(rng, rep, wl // 12) if noisy else rep
        return cat(junk, flank, rep, closing)
    while (len(closing) + wl) % 16 != i:                     # backward: closing + repeat + flank + junk
        wl += 1
    rep = repeat(mo, i, wl)
    if noisy:
        rep = edited(rng, rep, wl // 12)
        rep = rep[:wl] if len(rep) >= wl else cat(repeat(mo, i + 1, wl - len(rep)), rep)
    return cat(closing, rep, flank, junk)


def _grid():
    rng = np.random.RandomState(72)
    reads, what = [], []
    for l, locus in enumerate(LOCI):
        for slot in range(4):
            for i in range(16):
                reads.append(grid_read(rng, locus, slot, i, (i + l) % 2))
                what.append((l, slot, i))
    return reads, what


def _extra():
    rng = np.random.RandomState(73)
    junk = lambda lo, hi: rng.randint(0, 4, size=int(rng.randint(lo, hi + 1))).astype(np.uint8)      # noqa: E731
    A, M, B = LOCI[2]                                        # the 3-base motif
    A1, M1, B1 = LOCI[0]                                     # one base
    A17, M17, B17 = LOCI[8]
    A32, M32, B32 = LOCI[9]
    five = np.tile(M, 5)
    other = np.full(25, (int(M1[0]) + 1) & 3, np.uint8)
    return [
        cat(junk(3, 9), A, five, junk(20, 30), ref.revcomp(B), junk(3, 9)),        # A and rc B, both exact: slots 0 and 3 tie, slot 0 wins
        cat(junk(3, 9), B, five, A, np.tile(M, 7)),                                # the flanks in the wrong order: slots 0 and 1 tie
        ref.revcomp(cat(junk(3, 9), B, five, A, np.tile(M, 7))),                   # the same on the other strand: slots 2 and 3 tie, slot 2 wins
        cat(junk(5, 20), A),                                                       # an empty window at the read's end
        cat(B, junk(5, 20)),                                                       # and at its start
        ref.revcomp(cat(junk(5, 20), A)),
        cat(junk(0, 9), A17, M17[:16]), cat(junk(0, 9), A32, M32[:31]), cat(M32[3:], B32, junk(0, 9)),      # windows shorter than the motif
        cat(junk(0, 9), A32, M32[:1]), cat(junk(0, 9), A32, (M32[:1] + 1) & 3),
        cat(junk(0, 9), A1, other), cat(other[:12], B1, junk(0, 9)),               # windows without a positive cell
        cat(junk(0, 9), A, five, B, junk(0, 9)), ref.revcomp(cat(A17, np.tile(M17, 3), B17)),      # spanning rows
        cat(A32, np.tile(M32, 9)),                                                 # 288 rows of the largest bucket
        junk(150, 200), np.zeros(1, np.uint8),
    ]


GRID, GRID_WHAT = _grid()
EXTRA = _extra()
BATCH = GRID + EXTRA
assert max(len(r) for r in BATCH) <= 400

_WANT = {}


def want(K, scores=(1, 1, 1), priority=pref.SUB_LEFT_UP):
    """the reference columns of BATCH against LOCI, computed once and never changed"""
    key = (K, tuple(scores), priority)
    if key not in _WANT:
        cols = pref.genotype_partial(BATCH, LOCI, K, *scores, max_tail=MAX_TAIL, priority=priority)
        for c in cols:
            c.setflags(write=False)
        _WANT[key] = cols
    return _WANT[key]


def task_batch(tasks: int, seed: int = 0):
    """reads of which exactly `tasks` hold LOCI[2]'s left flank, exact, and some repeat after it - one task each, all of one variant - among
    reads that hold no flank; in a seeded shuffle"""
    rng = np.random.RandomState(900 + tasks + seed)
    A, M, _ = LOCI[2]
    reads = [cat(rng.randint(0, 4, size=int(rng.randint(0, 20))), A, repeat(M, t, 7 + t % 40)) for t in range(tasks)]
    reads += [rng.randint(0, 4, size=int(rng.randint(30, 80))).astype(np.uint8) for _ in range(5)]
    return [reads[k] for k in rng.permutation(len(reads))]
