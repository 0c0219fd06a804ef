"""Loci and reads for the catalogue genotype's tests, built per (K, q) from seeded generators: tests/test_catalog_ref.py shows from the
reference alone that they are not degenerate, tests/test_gpu_catalog.py runs them on the GPU.  Reads are of at most 400 bases."""
import numpy as np

from tests import motif_search_ref as ref

KQ = [(0, 16), (1, 8), (3, 8), (3, 16)]
MANY = 70                           # loci that share both flanks: one read is a candidate for all of them


def _cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts]).astype(np.uint8)


def _sub(p, at):
    """p with substitutions at the given places"""
    p = np.array(p, np.uint8)
    for a in at:
        p[a] = (p[a] + 1) & 3
    return p


def cases(K: int, q: int):
    """-> (loci, reads): loci = [(A, M, B)] of code arrays"""
    rng = np.random.RandomState(1000 * K + q)
    seq = lambda n: rng.randint(0, 4, size=n).astype(np.uint8)      # noqa: E731
    junk = lambda lo, hi: seq(int(rng.randint(lo, hi + 1)))         # noqa: E731
    need = (K + 1) * q
    lens = [need, min(need + 1, 64), 64]

    def motif(U):
        M = seq(U)
        while U > 1 and len(set(M.tolist())) == 1:
            M = seq(U)
        return M

    # loci 0..5: motifs either side of the lane/wave border, flanks of exactly need bases, of one more, and of 64
    loci = [(seq(lens[k % 3]), motif(U), seq(lens[(k + 1) % 3])) for k, U in enumerate((1, 3, 6, 16, 17, 40))]
    loci.append((loci[1][0], motif(4), seq(need)))                  # locus 6 shares its left flank with locus 1
    rep = np.tile(np.array([0, 1], np.uint8), q // 2)               # locus 7: the left flank's first seed is (AC) x q / 2
    loci.append((_cat(rep, seq(need - q)), motif(5), seq(need)))
    first_many = len(loci)
    A, B = seq(64), seq(64)
    loci += [(A, motif(2 + j % 7), B) for j in range(MANY)]         # the same flanks, different motifs
    reads = []
    for k, (A, M, B) in enumerate(loci[:first_many]):
        U = len(M)
        for c in (0, 2, min(30, 200 // U)):
            for strand in (0, 1):
                x = _cat(junk(0, 12), A, np.tile(M, c), B, junk(0, 12))
                reads.append(ref.revcomp(x) if strand else x)
        # K substitutions in the left flank, one in the middle of every seed but seed i: seed i alone survives
        for i in range(K + 1):
            hurt = _sub(A, [j * q + q // 2 for j in range(K + 1) if j != i])
            reads.append(_cat(junk(0, 9), hurt, np.tile(M, 3), B, junk(0, 9)))
    A, M, B = loci[1]
    five = np.tile(M, 5)
    A3, M3, B3 = loci[3]
    reads += [
        _cat(junk(5, 20), A[:q], seq(len(A) - q), five, B, junk(5, 9)),            # both sides seeded, the left flank beyond K
        _cat(junk(0, 9), B, five, A, junk(0, 9)),                                  # the flanks in the wrong order
        ref.revcomp(_cat(B, five, A)),
        _cat(junk(5, 20), A, five, junk(30, 40)),                                  # seeded on the left only
        ref.revcomp(_cat(junk(30, 40), five, B, junk(5, 20))),                     # on the right only
        _cat(junk(0, 9), A, five, ref.revcomp(B), junk(0, 9)),                     # A in orientation 0, B in orientation 1
        _cat(A, five, B, junk(20, 30), ref.revcomp(_cat(A, np.tile(M, 2), B))),    # both orientations valid, a tie: orientation 0
        _cat(A3, M3[:7], B3), _cat(A3, B3),                                        # a window shorter than its motif; an empty window
        seq(q - 1), seq(q), np.zeros(1, np.uint8), junk(100, 200),                 # shorter than a seed, exactly a seed, one base, no seed
    ]
    if K > 0:
        reads.append(_cat(_sub(A, [q // 2]), five, B, junk(20, 30), ref.revcomp(_cat(A, np.tile(M, 2), B))))      # both valid, the reverse one is nearer
    A7, M7, B7 = loci[7]
    reads.append(_cat(np.tile(np.array([0, 1], np.uint8), 40), A7[q:], np.tile(M7, 4), B7, junk(0, 9)))          # the seed (AC) x q / 2 at >= 20 places
    A, M, B = loci[first_many]
    reads += [_cat(junk(0, 9), A, np.tile(M, 6), B, junk(0, 9)), ref.revcomp(_cat(A, np.tile(loci[first_many + 3][1], 9), B))]
    assert max(len(r) for r in reads) <= 400
    return loci, reads


def count_cases(n: int):
    """-> (loci, reads): one locus and n reads of one candidate and one row each, so that reads[:k] has exactly k of both"""
    rng = np.random.RandomState(77)
    A, M, B = (rng.randint(0, 4, size=m).astype(np.uint8) for m in (40, 3, 36))
    M = np.array([1, 0, 2], np.uint8)
    reads = []
    for i in range(n):
        x = _cat(rng.randint(0, 4, size=i % 7), A, np.tile(M, 1 + i % 9), B, rng.randint(0, 4, size=i % 5))
        reads.append(ref.revcomp(x) if i % 3 == 1 else x)
    return [(A, M, B)], reads


BIG_LOCI, BIG_CARRIED, BIG_READS, BIG_K, BIG_Q = 100000, 10, 300, 3, 12


def big_catalog():
    """-> (A [n, 48], motifs, B [n, 48], reads, carried): 100 000 loci of random 48-base flanks, of which the `carried` ten are held by the 300
    reads (30 reads each, both strands); the other loci's flanks are random but for this: tests/test_catalog_ref.py shows that no read holds a seed of them"""
    rng = np.random.RandomState(2024)
    A = rng.randint(0, 4, size=(BIG_LOCI, 48)).astype(np.uint8)
    B = rng.randint(0, 4, size=(BIG_LOCI, 48)).astype(np.uint8)
    motifs = [np.array([(l >> 2 * t) & 3 for t in range(3)] + [3 - (l & 3)], np.uint8) for l in range(BIG_LOCI)]      # four bases, never a homopolymer
    carried = sorted(int(v) for v in rng.choice(BIG_LOCI, size=BIG_CARRIED, replace=False))
    reads = []
    for i in range(BIG_READS):
        l = carried[i % BIG_CARRIED]
        x = _cat(rng.randint(0, 4, size=i % 11), A[l], np.tile(motifs[l], 2 + i % 13), B[l], rng.randint(0, 4, size=i % 6))
        reads.append(ref.revcomp(x) if i % 4 == 3 else x)
    # a locus that is not carried and has a seed some read holds by chance (one 12-mer in ten is a seed) draws its flanks again
    held = np.unique(np.concatenate([codes_of(x[None, :], BIG_Q).ravel() for x in reads]))
    at = [i * BIG_Q for i in range(BIG_K + 1)]
    while True:
        hit = np.zeros(BIG_LOCI, bool)
        for F in (A, B):
            for P in (F, (3 - F)[:, ::-1]):
                hit |= np.isin(codes_of(P, BIG_Q)[:, at], held).any(axis=1)
        hit[carried] = False
        if not hit.any():
            break
        A[hit] = rng.randint(0, 4, size=(int(hit.sum()), 48))
        B[hit] = rng.randint(0, 4, size=(int(hit.sum()), 48))
    return A, motifs, B, reads, carried


def codes_of(rows, q):
    """the q-mer at every position of every row of a 2-D code array, as integers: [rows, len - q + 1]"""
    rows = np.asarray(rows, np.int64)
    return sum(rows[:, t:rows.shape[1] - q + 1 + t] << (2 * (q - 1 - t)) for t in range(q))
