"""tests/flank_ref.py - the flank search's definition as the GPU tests take it - against brute force: ed() of every substring of small random
texts, the tie rules on crafted ones, the strand rule, and the genotype's pairing rules on hand-made hits (CPU)."""
import numpy as np

from tests import flank_ref as fref
from tests import motif_search_ref as ref


def test_hits_equal_brute_force_on_small_cases():
    rng = np.random.RandomState(5)
    n = 0
    for m in (1, 2, 3, 5, 7):
        for _ in range(12):
            p = rng.randint(0, 2 + rng.randint(0, 3), size=m)
            reads = [rng.randint(0, 2 + rng.randint(0, 3), size=int(rng.randint(0, 15))) for _ in range(9)] + [np.zeros(0, np.int64), p.copy(), p[:-1].copy()]
            dist, start, end = fref.hits(reads, p)
            for r, x in enumerate(reads):
                assert (int(dist[r]), int(start[r]), int(end[r])) == fref.brute(list(p), list(x)), (list(p), list(x))
                n += 1
    assert n >= 700


def test_the_tie_rules():
    c = ref.codes_of
    # two exact copies: the first one's end; a run longer than the pattern: the smallest end, and from there the largest start
    d, s, e = fref.hits([c("TTACGTTTACGTT"), c("AAAA"), c("CCA"), c("G"), c("")], c("ACG"))
    assert (d[0], s[0], e[0]) == (0, 2, 5)
    assert (d[3], s[3], e[3]) == (2, 0, 1) and (d[4], s[4], e[4]) == (3, 0, 0)
    d, s, e = fref.hits([c("AAAA"), c("CCA")], c("AA"))
    assert (d[0], s[0], e[0]) == (0, 0, 2)
    d, s, e = fref.hits([c("CCA")], c("CA"))
    assert (d[0], s[0], e[0]) == (0, 1, 3)
    # one edit either way: ACGT against ACT (a deletion) - the shortest substring at the smallest end
    d, s, e = fref.hits([c("GGACTGG")], c("ACGT"))
    assert d[0] == 1 and (int(d[0]), int(s[0]), int(e[0])) == fref.brute(list(c("ACGT")), list(c("GGACTGG")))
    # nothing of the read helps: dist = m at end 0
    d, s, e = fref.hits([c("TTTT")], c("AC"))
    assert (d[0], s[0], e[0]) == (2, 0, 0)


def test_the_strand_rule():
    c = ref.codes_of
    reads = [c("TTACGGTT"), c("TTCCGTTT"), c("TTTTTTTT"), c("ACGT")]
    dist, start, end, strand = fref.search(reads, [c("ACGG"), c("ACGT")])
    assert dist[:2, 0].tolist() == [0, 0] and strand[:2, 0].tolist() == [0, 1]          # CCGT is ACGG's reverse complement
    assert (start[1, 0], end[1, 0]) == (2, 6)
    assert strand[:, 1].tolist() == [0, 0, 0, 0]                                        # a palindrome: a tie everywhere, the forward pattern wins
    fwd = fref.search(reads, [c("ACGG")], both_strands=False)
    assert fwd[3].sum() == 0 and fwd[0][1, 0] > 0
    assert all(a.dtype == np.int32 for a in fwd[:3]) and fwd[3].dtype == np.uint8 and fwd[0].shape == (4, 1)


def test_the_pairing_rules():
    far = (9, 0, 0)
    # orientation 0 alone, then orientation 1 alone: the window between the flanks, each distance named by the locus' flank
    assert fref.pair((1, 2, 10), (0, 25, 33), far, far, 1) == (1, 0, 1, 0, 10, 25)
    assert fref.pair(far, far, (2, 40, 50), (1, 5, 12), 2) == (1, 1, 2, 1, 12, 40)
    # an empty window spans; flanks that overlap by one base do not
    assert fref.pair((0, 2, 10), (0, 10, 18), far, far, 0) == (1, 0, 0, 0, 10, 10)
    assert fref.pair((0, 2, 10), (0, 9, 18), far, far, 0) == (0, 0, 0, 0, 0, 0)
    assert fref.pair(far, far, (0, 9, 18), (0, 2, 10), 0) == (0, 0, 0, 0, 0, 0)
    # a flank beyond K
    assert fref.pair((2, 2, 10), (0, 25, 33), far, far, 1) == (0, 0, 0, 0, 0, 0)
    assert fref.pair((2, 2, 10), (0, 25, 33), far, far, 2)[0] == 1
    # both valid: the smaller sum, orientation 0 on a tie
    assert fref.pair((1, 2, 10), (1, 25, 33), (0, 40, 50), (1, 5, 12), 3)[:2] == (1, 1)
    assert fref.pair((1, 2, 10), (0, 25, 33), (0, 40, 50), (1, 5, 12), 3) == (1, 0, 1, 0, 10, 25)


def test_genotype_columns_of_a_hand_made_batch():
    c = ref.codes_of
    A, M, B = c("ACGTTGCA"), c("CAG"), c("TTGACCGA")
    fwd = np.concatenate([c("GG"), A, np.tile(M, 4), B, c("GG")])
    empty = np.concatenate([A, B])
    reads = [fwd, ref.revcomp(fwd), empty, np.concatenate([c("GG"), B, np.tile(M, 4), A]), np.concatenate([A, np.tile(M, 4)])]
    (sp, o, fd, w, f, sc, ra), why = fref.genotype(reads, [(A, M, B)], 0)
    assert sp[:, 0].tolist() == [1, 1, 1, 0, 0] and o[:, 0].tolist() == [0, 1, 0, 0, 0]
    assert w[0, 0].tolist() == [10, 22] and w[1, 0].tolist() == [10, 22] and w[2, 0].tolist() == [8, 8]
    assert f[0, 0].tolist() == [10, 21, 12, 4, 12, 0, 0, 0] and f[1, 0].tolist() == [10, 21, 12, 4, 12, 0, 0, 0] and sc[0, 0] == 12 and ra[0, 0] == 1.0
    assert f[2, 0].tolist() == [0] * 8 and sc[2, 0] == 0 and ra[2, 0] == 0
    assert why == [(3, 0, "order"), (4, 0, "right")]
    assert fd.shape == (5, 1, 2) and not fd.any() and not f[3:].any() and not w[3:].any()
