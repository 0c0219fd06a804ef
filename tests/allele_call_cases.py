"""The inputs of the allele calls' tests, shared by the CPU tests (tests/test_allele_call_ref.py: the reference on them is not degenerate) and the
GPU tests (tests/test_gpu_allele_call.py: the library equals the reference on them).  Every input is a Rows of numpy columns, shaped and typed
as mtr_amd.Genotypes' spanning, window, fields and ratio - the four columns the call reads - and every builder is seeded."""
from typing import NamedTuple

import numpy as np

from tests import motif_search_ref as ref

MIN_RATIO = 0.7                     # what the built inputs' dropped rows lie under and their supporting rows at or over
SWEEP = ((1, 0, 1), (3, 20, 2), (2, 50, 5))      # (min_support, min_percent, min_sep)
TILE = 256                          # AL_TILE = AL_BLOCK of mtr_amd/csrc/allele_call.hip.inc; its other constant is the wavefront's 64 lanes
# 0 .. 3, then one below, at and one above: the wavefront, the tile, two tiles, four tiles; eight tiles and one; n_reads itself
EDGE_SUPPORT = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 512, 1023, 1024, 1025, 2049, 3000)
EDGE_READS = 3000
BIG_WINDOW = 2_500_000              # the last edge locus' windows reach this, so that its cost1 passes 2^31 (see tile_edges)


class Rows(NamedTuple):
    spanning: np.ndarray            # uint8 [n, m]
    window: np.ndarray              # int32 [n, m, 2]
    fields: np.ndarray              # int32 [n, m, 8]
    ratio: np.ndarray               # float32 [n, m]


def garbage(rng, n, m):
    """rows that span nothing and hold garbage in every other column: negative windows and copies, ratios over 1, below 0 and NaN"""
    ratio = rng.uniform(-2, 2, size=(n, m)).astype(np.float32)
    ratio[rng.rand(n, m) < 0.1] = np.nan
    return Rows(np.zeros((n, m), np.uint8), rng.randint(-2 ** 31, 2 ** 31 - 1, size=(n, m, 2)).astype(np.int32),
                rng.randint(-2 ** 31, 2 ** 31 - 1, size=(n, m, 8)).astype(np.int32), ratio)


def put(rows, rng, read, locus, copies, bases, ratio=None):
    """read supports locus with these copies and a window of these bases"""
    lo = int(rng.randint(0, 1000))
    rows.spanning[read, locus] = 1
    rows.window[read, locus] = (lo, lo + int(bases))
    rows.fields[read, locus] = (lo, lo + int(bases) - 1, int(bases), int(copies), int(bases), 0, 0, 0)
    rows.ratio[read, locus] = np.float32(rng.uniform(MIN_RATIO, 1.0)) if ratio is None else np.float32(ratio)
    if bases > 0 and ratio is None and rng.rand() < 0.2:
        rows.ratio[read, locus] = np.float32(MIN_RATIO)                # exactly the bound, in float32: kept


def drop(rows, rng, read, locus):
    """read spans locus with a non-empty window and a ratio under MIN_RATIO: not supporting, whatever its values - negative ones too"""
    lo = int(rng.randint(0, 1000))
    rows.spanning[read, locus] = 1
    rows.window[read, locus] = (lo, lo + int(rng.randint(1, 500)))
    rows.fields[read, locus] = rng.randint(-50, 50, size=8)
    below = np.nextafter(np.float32(MIN_RATIO), np.float32(0))
    rows.ratio[read, locus] = below if rng.rand() < 0.5 else np.float32(rng.uniform(0, 0.69))


def pattern(rng, kind, count):
    """count copies values in read order: two noisy clusters; all equal (ties fall to the read order); strictly descending in read order (the
    fill order is nowhere the sorted order); stutter around one value"""
    if kind == "clusters":
        return np.where(rng.rand(count) < 0.4, 35, 20) + rng.randint(-2, 3, size=count)
    if kind == "equal":
        return np.full(count, 17)
    if kind == "descending":
        return 5000 - np.arange(count)
    assert kind == "stutter"
    return 30 + rng.choice([-1, 0, 0, 0, 0, 0, 1], size=count)


KINDS = ("clusters", "equal", "descending", "stutter")


def tile_edges():
    """3000 reads x 16 loci with EDGE_SUPPORT supporting reads, the four patterns in turn, a motif of 3 + locus % 4 bases with a jitter of a few
    bases, a tenth of the other rows dropped by the ratio, the rest garbage.  The last locus, every read supporting, has windows in two noisy
    clusters near 100 000 and near BIG_WINDOW bases: a cost1 over 2^31 needs 3000 windows further apart than the longest read's 833 333 bases
    allow (at most 1500 x 833 333 = 1.25e9), and the call puts no bound on a window - so the rows' windows are that far apart."""
    rng = np.random.RandomState(20261)
    n, m = EDGE_READS, len(EDGE_SUPPORT)
    rows = garbage(rng, n, m)
    for l, count in enumerate(EDGE_SUPPORT):
        who = np.sort(rng.choice(n, size=count, replace=False))
        copies = pattern(rng, KINDS[l % 4] if l < m - 1 else "clusters", count)
        unit = 3 + l % 4
        bases = copies * unit + rng.randint(-1, 2, size=count) * (KINDS[l % 4] != "equal")
        if l == m - 1:
            bases = np.where(copies > 27, BIG_WINDOW - 40_000, 100_000) + rng.randint(0, 40_000, size=count)
        for r, c, b in zip(who, copies, bases):
            put(rows, rng, r, l, c, b)
        rest = np.setdiff1d(np.arange(n), who)
        for r in rest[rng.rand(len(rest)) < 0.1]:
            drop(rows, rng, r, l)
    return rows


def many_loci(swap=False):
    """40 reads x 700 loci, most of them empty, the first one empty and the last one not; swap: the loci in reverse order"""
    rng = np.random.RandomState(20262)
    n, m = 40, 700
    rows = garbage(rng, n, m)
    for l in list(np.nonzero(rng.rand(m) < 0.15)[0]) + [m - 1]:
        if l == 0:
            continue
        who = np.nonzero(rng.rand(n) < rng.choice([0.05, 0.3, 0.9]))[0]
        copies = pattern(rng, KINDS[l % 4], len(who))
        for r, c in zip(who, copies):
            put(rows, rng, r, l, c, c * 4 + rng.randint(0, 3))
    put(rows, rng, 7, m - 1, 9, 36)
    drop(rows, rng, 3, 0)
    assert rows.spanning[:, 0].sum() == 1 and rows.spanning[:, m - 1].sum() >= 1
    return Rows(*[np.ascontiguousarray(c[:, ::-1]) for c in rows]) if swap else rows


def lane_edges(m):
    """70 reads x m loci, m = 63, 64, 65: either side of the loci count from which every lane counts for itself"""
    rng = np.random.RandomState(20263 + m)
    n = 70
    rows = garbage(rng, n, m)
    for l in range(m):
        who = np.nonzero(rng.rand(n) < (0.0 if l % 7 == 3 else 0.6))[0]
        for r, c in zip(who, pattern(rng, KINDS[l % 4], len(who))):
            put(rows, rng, r, l, c, c * 2)
    return rows


SPREAD_LOCI = 4096                  # AL_SPREAD_LOCI: up to this many loci the kernels keep the loci's counters 256 bytes apart


def spread_edges(m):
    """12 reads x m loci, m = 4096, 4097: either side of the loci count up to which the counters are spread"""
    rng = np.random.RandomState(20267 + m)
    n = 12
    rows = garbage(rng, n, m)
    for l in range(m):
        who = np.nonzero(rng.rand(n) < (0.0 if l % 5 == 2 else 0.5))[0]
        for r, c in zip(who, pattern(rng, KINDS[l % 4], len(who))):
            put(rows, rng, r, l, c, c * 3)
    return rows


# hand-worked lists (tests/test_allele_call_ref.py says what each is for); under from_lists a value is the copies, and 3 x the value the bases
HAND = ([19, 20, 20, 20, 20, 21, 34, 35, 35, 35, 36], [10] * 9 + [40], [10, 10, 10, 40, 40, 40, 70, 70, 70], [], [5], [4, 9], [7] * 6,
        [5, 5, 9, 9, 9], [1, 1, 2, 2], [0, 0, 0, 0, 12, 12, 13])


def from_lists(lists=HAND, seed=20264):
    """one locus per list, its values dealt to random reads in random order; every other row garbage, two reads dropped by the ratio"""
    rng = np.random.RandomState(seed)
    n, m = max(len(v) for v in lists) + 3, len(lists)
    rows = garbage(rng, n, m)
    for l, v in enumerate(lists):
        who = rng.permutation(n)
        for r, c in zip(who, v):
            put(rows, rng, r, l, c, 3 * c)
        for r in who[len(v):len(v) + 2]:
            drop(rows, rng, r, l)
    return rows


def empty_windows():
    """5 reads x 1 locus for min_ratio = 1: three alleles of no copies (an empty window, ratio 0) stay, a perfect repeat stays, an imperfect one
    goes"""
    rng = np.random.RandomState(20265)
    rows = garbage(rng, 5, 1)
    for r in (0, 2, 3):
        put(rows, rng, r, 0, 0, 0, ratio=0.0)
    put(rows, rng, 1, 0, 6, 18, ratio=1.0)
    put(rows, rng, 4, 0, 6, 18, ratio=np.nextafter(np.float32(1), np.float32(0)))
    return rows


def smallest(supported):
    rng = np.random.RandomState(20266)
    rows = garbage(rng, 1, 1)
    if supported:
        put(rows, rng, 0, 0, 11, 33)
    return rows


# ---- end to end: reads, two loci -----------------------------------------------------------------------------------------------------------
E2E_SEED = 7
E2E_K, E2E_MIN_RATIO, E2E_RULE = 2, 0.7, (3, 20, 2)


def e2e():
    """-> (reads, loci): locus 0 = (flank 20, motif of 3, flank 24) with 9 reads of 5 copies and 7 of 12, locus 1 the same shape with a motif
    of 6 and 6 reads of 8 copies; single reads at +/- 1 copy, flanks and repeats lightly edited, strands alternating; four junk reads.  Code
    arrays, some 100 bases a read."""
    rng = np.random.RandomState(E2E_SEED)

    def edited(p, edits):
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

    cat = lambda *p: np.concatenate([np.asarray(x, np.uint8) for x in p]).astype(np.uint8)      # noqa: E731
    junk = lambda lo, hi: rng.randint(0, 4, size=int(rng.randint(lo, hi + 1))).astype(np.uint8)      # noqa: E731
    loci = []
    for U in (3, 6):
        M = rng.randint(0, 4, size=U).astype(np.uint8)
        while len(set(M.tolist())) == 1:
            M = rng.randint(0, 4, size=U).astype(np.uint8)
        loci.append((rng.randint(0, 4, size=20).astype(np.uint8), M, rng.randint(0, 4, size=24).astype(np.uint8)))
    reads = []
    for k, plan in enumerate(([(5, 9), (12, 7)], [(8, 6)])):
        A, M, B = loci[k]
        for c, cnt in plan:
            for i in range(cnt):
                cc = c + (1 if i == 3 else -1 if i == 5 else 0)       # stutter
                rep = edited(np.tile(M, cc), i % 2)
                x = cat(junk(0, 12), edited(A, i % 3 == 0), rep, edited(B, i % 3 == 1), junk(0, 12))
                reads.append(ref.revcomp(x) if i % 2 else x)
    reads += [junk(60, 90) for _ in range(4)]
    assert max(len(r) for r in reads) <= 128          # 12 + 21 + 9 x 6 + 1 + 25 + 12 at the most
    return reads, loci
