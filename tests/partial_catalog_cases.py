"""Loci and reads for the tests of the partial genotype at catalogue scale, from seeded generators: tests/test_partial_catalog_ref.py shows from
the references alone that they are not degenerate, tests/test_gpu_partial_catalog.py runs them on the GPU.  Reads are of at most 400 bases.

GRID_KQ   (i)   tests/partial_cases.py's BATCH x LOCI, whose flanks of 20 .. 24 bases take (K, q) = (0, 16), (1, 8), (1, 10).
cases()   (ii)  for (K, q) = (3, 8) and (3, 16): flanks of exactly (K + 1) q bases, of one more and of 64; motifs of 1, 4, 5, 8, 9, 16, 17 and 32
                bases; every slot of every locus exact and with K substitutions that leave one seed; spanning reads, ties, empty windows, windows
                without a positive cell, a seeded flank beyond K, and MANY loci that share their flanks.
mixed()   (iii) one bucket's launch of several wavefronts in which every lane has a motif, a length and a direction of its own.
count_cases() (iv) reads[:k] has exactly k rows.
big_cut() (v)   tests/catalog_cases.py's 100 000 loci with its reads cut inside the repeat."""
import numpy as np

from tests import catalog_cases as cc
from tests import motif_search_ref as ref
from tests import partial_cases as pc

GRID_KQ = [(0, 16), (1, 8), (1, 10)]
GRID_COUNTS = {(0, 16): (396, 341), (1, 8): (671, 510), (1, 10): (607, 510)}      # (K, q): candidates, partial rows of the dense reference
KQ = [(3, 8), (3, 16)]
US = (1, 4, 5, 8, 9, 16, 17, 32)
MANY = 70
MAX_TAIL = 10

_cat = pc.cat


def _motif(rng, U):
    M = rng.randint(0, 4, size=U).astype(np.uint8)
    while U > 1 and len(set(M.tolist())) == 1:
        M = rng.randint(0, 4, size=U).astype(np.uint8)
    return M


def slot_read(rng, locus, slot, flank=None, window=40, phase=0, closing=0, junk=6):
    """a read that holds slot `slot`'s pattern of the locus (or `flank` in its place, given as the A or B it stands for) next to `window` bases
    of the repeat starting at `phase`, then `closing` other bases; `junk` bases outside the flank.  Slots 2 and 3 are the reverse complements of
    a slot-0 and a slot-1 read"""
    A, M, B = locus
    side = slot in (1, 3)                                    # the read holds B (or rc B)
    F = (B if side else A) if flank is None else flank
    rep, close, jk = pc.repeat(M, phase, window), rng.randint(0, 4, size=closing).astype(np.uint8), rng.randint(0, 4, size=junk).astype(np.uint8)
    x = _cat(close, rep, F, jk) if side else _cat(jk, F, rep, close)
    return ref.revcomp(x) if slot >= 2 else x


def cases(K: int, q: int):
    """-> (loci, reads) of case (ii); loci = [(A, M, B)] of code arrays"""
    rng = np.random.RandomState(5000 + 100 * K + q)
    seq = lambda n: rng.randint(0, 4, size=n).astype(np.uint8)      # noqa: E731
    need = (K + 1) * q
    lens = [need, min(need + 1, 64), 64]
    loci = [(seq(lens[k % 3]), _motif(rng, U), seq(lens[(k + 1) % 3])) for k, U in enumerate(US)]
    first_many = len(loci)
    A, B = seq(64), seq(64)
    loci += [(A, _motif(rng, 1 + j % 32), B) for j in range(MANY)]      # the same flanks, motifs of every length: one read is a candidate of all
    reads = []
    for k, locus in enumerate(loci[:first_many]):
        U = len(locus[1])
        for slot in range(4):
            F = locus[0] if slot in (0, 2) else locus[2]
            reads.append(slot_read(rng, locus, slot, window=30 + 7 * slot + k, phase=k + slot, junk=3 + slot))
            # K substitutions, one in the middle of every seed but seed i: seed i alone survives
            i = (k + slot) % (K + 1)
            hurt = cc._sub(F, [j * q + q // 2 for j in range(K + 1) if j != i])
            reads.append(slot_read(rng, locus, slot, flank=hurt, window=50 + 3 * k, phase=slot, closing=20 * (k % 2), junk=5))
        reads.append(_cat(seq(4), locus[0], np.tile(locus[1], max(1, 12 // U)), locus[2], seq(5)))                  # spanning
        reads.append(ref.revcomp(_cat(seq(2), locus[0], np.tile(locus[1], max(2, 20 // U)), locus[2])))             # spanning, the other strand
    A, M, B = loci[1]
    A1, M1, B1 = loci[0]
    other = np.full(25, (int(M1[0]) + 1) & 3, np.uint8)
    reads += [
        _cat(seq(7), A[:q], seq(len(A) - q), np.tile(M, 6)),                      # slot 0 seeded and beyond K: a candidate, no row
        _cat(seq(5), A, np.tile(M, 5), seq(25), ref.revcomp(B), seq(4)),          # A and rc B both exact: slots 0 and 3 tie, slot 0 wins
        _cat(seq(5), B, np.tile(M, 5), A, np.tile(M, 7)),                         # the flanks in the wrong order: slots 0 and 1 tie
        ref.revcomp(_cat(seq(5), B, np.tile(M, 5), A, np.tile(M, 7))),            # slots 2 and 3 tie, slot 2 wins
        _cat(seq(5), cc._sub(A, [q // 2]), np.tile(M, 5), seq(25), ref.revcomp(B)),      # slot 3 exact, slot 0 at distance 1: the chosen slot is not the lowest
        _cat(seq(9), A), _cat(B, seq(9)), ref.revcomp(_cat(seq(9), A)),           # empty windows
        _cat(seq(3), A1, other), _cat(other[:12], B1, seq(3)),                    # windows without a positive cell
        seq(q - 1), seq(q), np.zeros(1, np.uint8), seq(150),
    ]
    A, M, B = loci[first_many]
    reads += [_cat(seq(3), A, np.tile(M, 30)), ref.revcomp(_cat(np.tile(loci[first_many + 5][1], 9), B, seq(6))),      # candidates of all MANY loci
              _cat(seq(3), A, np.tile(loci[first_many + 31][1], 3), B)]                                                # spanning for all of them
    assert max(len(r) for r in reads) <= 400
    return loci, reads


# The edits of the reads behind the last full 64 (the lanes of a launch's last, partial wavefront where the tasks are appended in order) come from a
# generator of their own, seeded so that one of those rows depends on the predecessor's order: tests/test_partial_catalog_ref.py checks that it does.
TAIL_NOISE = {(5, 130): 22, (17, 70): 0}
SET_SEED = {(17, 70): 2}                                # likewise the set's own generator, for the rows of the full stretches of 64


def mixed(first_u: int, last_u: int, n_loci: int, seed: int = 0, tail_seed=None):
    """-> (loci, reads, what) of case (iii): n_loci loci with distinct flanks of 24 bases and motifs of first_u .. last_u bases in turn, one read
    each: read i holds slot i % 4 of locus i, exact, and a window of 7 .. 110 bases that begins (forward slots) or ends (backward slots, whose
    windows begin at base 0) at every residue of a word, with substitutions, insertions and deletions in the longer ones.  K = 0 and q = 12 are meant: every
    read is one candidate, one row and one task, and 64 consecutive tasks of the bucket's list are 64 different motifs in both directions.
    what[i] = (locus, slot, window length)"""
    rng = np.random.RandomState(3100 + first_u + seed + SET_SEED.get((first_u, n_loci), 0))
    tail = np.random.RandomState(TAIL_NOISE.get((first_u, n_loci), 0) if tail_seed is None else tail_seed)
    seq = lambda n: rng.randint(0, 4, size=n).astype(np.uint8)      # noqa: E731
    loci, reads, what = [], [], []
    for i in range(n_loci):
        U = first_u + i % (last_u - first_u + 1)
        M = _motif(rng, U)
        while any(np.array_equal(M, o[1]) for o in loci):    # every locus a motif of its own
            M = _motif(rng, U)
        locus = (seq(24), M, seq(24))
        slot = i % 4
        res = (i // 4) % 16
        wl = 7 + 16 * min((i // 4 + slot + 3) % 7, (103 - res) // 16) + res     # 7 .. 110 bases; a slot's windows end at every residue
        A, M, B = locus
        rep = pc.repeat(M, i, wl)
        if wl >= 20:                                         # edits of every kind, the length kept at the end away from the flank
            rep = pc.edited(tail if i >= n_loci - n_loci % 64 else rng, rep, wl // 12)
            more = pc.repeat(M, i + 3, max(0, wl - len(rep)))
            rep = _cat(more, rep)[-wl:] if slot in (1, 3) else _cat(rep, more)[:wl]
        pad = seq(((i // 4) % 16 - 24) % 16 if slot in (0, 3) else i % 5)      # a forward window begins at len(pad) + 24
        x = _cat(rep, B, pad) if slot in (1, 3) else _cat(pad, A, rep)          # built on the strand of slots 0 and 1 ..
        x = ref.revcomp(x) if slot >= 2 else x                                  # .. and turned for slots 2 and 3
        loci.append(locus); reads.append(x); what.append((i, slot, wl))
    return loci, reads, what


def count_cases(n: int):
    """-> (loci, reads) of case (iv): two loci and n reads of one candidate, one row and one task each - reads[:k] has exactly k of all three; K = 2
    and q = 12 are meant"""
    rng = np.random.RandomState(78)
    seq = lambda m: rng.randint(0, 4, size=m).astype(np.uint8)      # noqa: E731
    loci = [(seq(40), np.array([1, 0, 2], np.uint8), seq(36)), (seq(36), np.array([3, 1, 0, 0, 2, 1, 3], np.uint8), seq(40))]
    reads = [slot_read(rng, loci[i % 2], i % 4, window=9 + i % 40, phase=i, closing=12 * (i % 3 == 0), junk=i % 7) for i in range(n)]
    return loci, reads


def big_cut():
    """-> (A, motifs, B, reads, carried) of case (v): tests/catalog_cases.py's big_catalog() with every read cut inside its repeat - reads
    0 .. 3 of every eight to the prefix that keeps the first flank and one copy, reads 4 .. 7 to the suffix that keeps the last flank and one copy; every
    fourth read lies on the other strand, so all four slots occur.  A substring
    holds a subset of its read's q-mers: no cut read holds a seed of a locus that is not carried (tests/test_partial_catalog_ref.py checks it)"""
    A, motifs, B, reads, carried = cc.big_catalog()
    cut = []
    for i, x in enumerate(reads):
        front, back = i % 11, i % 6                          # big_catalog's junk before and behind; a turned read has them the other way round
        if i % 4 == 3:
            front, back = back, front
        keep = front + 48 + 4 + i % 4                        # the flank, one copy and up to three bases
        cut.append(x[:keep] if i % 8 < 4 else x[len(x) - (back + 48 + 4 + i % 4):])
    return A, motifs, B, cut, carried
