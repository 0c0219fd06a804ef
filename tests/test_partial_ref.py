"""tests/partial_ref.py - the partial genotype's definition (include/mtr_hip.h) in Python - held to extensions worked by hand, and the seeded
inputs of tests/partial_cases.py shown, from the reference alone, to be none of them degenerate: what the GPU tests compare is worth comparing."""
import numpy as np

from tests import flank_ref as fref
from tests import partial_cases as pc
from tests import partial_ref as pref


def _c(text):
    return ["ACGT".index(ch) for ch in text]


def test_extensions_worked_by_hand():
    """(ext_len, motif_bases, matches, score)"""
    ext = lambda y, m, *s, **kw: pref.extend(_c(y), _c(m), *s, **kw)      # noqa: E731
    assert ext("ACGACG", "ACG") == (6, 6, 6, 6)
    assert ext("GACGA", "ACG") == (5, 5, 5, 5)                           # the phase at the flank is free: the extension begins at the motif's G
    assert ext("ACGTT", "ACG") == (3, 3, 3, 3)                           # the first strict maximum: the repeat ends, two bases are the tail
    assert ext("TT", "A") == (0, 0, 0, 0) and ext("", "ACG") == (0, 0, 0, 0)
    # AC-ACG: the motif's G is deleted (left, -1): six motif bases on five read bases, five matches
    assert ext("ACACG", "ACG") == (5, 6, 5, 4) and ext("ACACG", "ACG", 2, 3, 2) == (5, 6, 5, 8)
    # ACtGACG: the t is an insertion (up, -1): six motif bases on seven read bases
    assert ext("ACTGACG", "ACG") == (7, 6, 6, 5)
    # anchored: no maximum with 0.  TTTTACGACG against ACG pays for its four leading bases; a local alignment would score 6
    assert ext("TTTTACGACG", "ACG") == (10, 10, 6, 2)
    assert ext("TTTTTTTACGACG", "ACG") == (0, 0, 0, 0)
    # the tie rule.  CAA against AA, row 1, column 1: sub = 0 - 1 and up = 0 - 1; sub comes first, so the C is a mismatch and consumes a motif
    # base: H(1, .) = -1 with C = 1; row 2: sub from H(1, 2) gives 0 with C = 2, T = 1; row 3: 1 with C = 3, T = 2.  With up first the C would be
    # an insertion and C = 2
    assert ext("CAA", "AA") == (3, 3, 2, 1) and ext("CAA", "AA", priority=pref.UP_LEFT_SUB) == (3, 2, 2, 1)
    # column 1 has no left term: against ACG the base G (row 1) reaches column 1 only by sub (-1) or up (-1), never from column 3 of its own row
    assert ext("G", "ACG") == (1, 1, 1, 1) and ext("GG", "GA", 1, 1, 1) == (1, 1, 1, 1)


def test_the_choice_of_slot_and_the_windows():
    far, L = (9, 0, 0), 100
    hit = lambda d, s, e: (d, s, e)      # noqa: E731
    assert pref.choose([hit(0, 10, 30), far, far, far], 3, L) == (0, 0, 30, L)
    assert pref.choose([far, hit(1, 60, 80), far, far], 3, L) == (1, 1, 0, 60)
    assert pref.choose([far, far, hit(2, 60, 80), far], 3, L) == (2, 2, 0, 60)
    assert pref.choose([far, far, far, hit(3, 10, 30)], 3, L) == (3, 3, 30, L)
    assert pref.choose([far, far, far, hit(4, 10, 30)], 3, L) is None                                   # no flank within K
    assert pref.choose([hit(0, 10, 30), hit(0, 60, 80), far, far], 3, L) is None                        # spanning: the genotype's row
    assert pref.choose([hit(1, 60, 80), hit(1, 10, 30), far, far], 3, L) == (0, 1, 80, L)               # the wrong order; a tie: the lowest slot
    assert pref.choose([hit(2, 60, 80), hit(1, 10, 30), far, hit(1, 5, 25)], 3, L) == (1, 1, 0, 10)     # the smallest dist, then the lowest slot
    assert pref.choose([hit(0, 80, 100), far, far, far], 0, L) == (0, 0, L, L)                          # an empty window


def test_one_row_by_hand():
    A, M, B = _c("ACGTTGCAAGGCTA"), _c("CAG"), _c("TTGACCGATACCGG")
    x = np.array(_c("GG") + A + _c("CAGCAGCTGCAGCA"), np.uint8)           # one mismatch, the read ends inside a copy
    cols = pref.genotype_partial([x, x[::-1].copy()], [(A, M, B)], 0, max_tail=0)
    partial, slot, fdist, window, ext, ratio, is_open = [c[0, 0].tolist() for c in cols]
    assert (partial, slot, fdist, window, is_open) == (1, 0, 0, [16, 30], 1)
    assert ext == [14, 14, 4, 13, 12, 0] and ratio == float(np.float32(13) / np.float32(14))
    assert all(not c[1, 0].any() for c in cols)                           # the reversed read holds no flank: a row of zeros
    # the same locus from the other strand: slot 2, the window before rc A, walked backwards against rc M
    from tests import motif_search_ref as ref
    cols = pref.genotype_partial([ref.revcomp(x)], [(A, M, B)], 0, max_tail=0)
    assert [c[0, 0].tolist() for c in cols][:5] == [1, 2, 0, [0, 14], [14, 14, 4, 13, 12, 0]]


def test_the_seeded_inputs_are_not_degenerate():
    U = np.array(pc.US)
    for K in pc.KS:
        partial, slot, fdist, window, ext, ratio, is_open = pc.want(K)
        n = window[:, :, 1] - window[:, :, 0]
        on = partial == 1
        assert all(int((on & (slot == s) & (U[None, :] == u)).sum()) >= 4 for s in range(4) for u in pc.US), K      # every slot, for every motif length
        assert int((on & (is_open == 1) & (n > 0)).sum()) >= 100 and int((on & (is_open == 0)).sum()) >= 50
        assert int((on & (n == 0)).sum()) >= 3 and int((on & (n > 0) & (n < U[None, :])).sum()) >= 3
        assert int((on & (n > 0) & (ext[:, :, 0] == 0)).sum()) >= 2                                     # windows without a positive cell
        assert (fdist.max() > 0) == (K > 0) and not (~on & ((slot != 0) | (fdist != 0) | (n != 0) | (is_open != 0))).any()
        assert int(n.max()) > 64 * 4                                                                    # (beyond MTR_TEST_MOTIF_LANE_ROWS=64 by far)
        # windows starting and ending at every residue of a word, in both directions (a backward window starts at hi and ends at base 0)
        for s in range(4):
            rows = on & (slot == s)
            assert {int(v) % 16 for v in window[:, :, 1][rows]} == set(range(16)), (K, s)
            assert {int(v) % 16 for v in window[:, :, 0][rows]} == (set(range(16)) if s in (0, 3) else {0}), (K, s)
    partial, slot, fdist, window, ext, *_ = pc.want(3)
    g = len(pc.GRID)
    # ties of dist between slots: the reads built for it, checked on the flank hits themselves
    A, M, B = pc.LOCI[2]
    from tests import motif_search_ref as ref
    for r, (tied, won) in zip(range(g, g + 3), (((0, 3), 0), ((0, 1), 0), ((2, 3), 2))):
        d = [int(fref.hits([pc.BATCH[r]], q)[0][0]) for q in (A, B, ref.revcomp(A), ref.revcomp(B))]
        assert d[tied[0]] == d[tied[1]] == 0 and partial[r, 2] == 1 and slot[r, 2] == won, (r, d)
    # spanning rows next to partial ones: zeros here, and the genotype's reference says spanning
    (sp, *_), _ = fref.genotype(pc.BATCH[g + 13:g + 15], pc.LOCI, 3)
    assert sp[0, 2] == 1 and sp[1, 8] == 1 and partial[g + 13, 2] == 0 and partial[g + 14, 8] == 0 and partial[g + 12].any()


def test_every_bucket_depends_on_the_predecessor_priority():
    """with the priority reversed (up, left, sub) motif_bases or matches change in rows of every bucket: the tie rule is tested"""
    ext, other = pc.want(3)[4], pc.want(3, (1, 1, 1), pref.UP_LEFT_SUB)[4]
    differs = ((ext[:, :, 1] != other[:, :, 1]) | (ext[:, :, 3] != other[:, :, 3])).sum(axis=0)
    per_bucket = {ub: int(sum(d for d, u in zip(differs, pc.US) if lo < u <= ub)) for lo, ub in ((0, 4), (4, 8), (8, 16), (16, 32))}
    print(per_bucket)
    assert all(v >= 2 for v in per_bucket.values()), per_bucket
    assert np.array_equal(ext[:, :, 0], other[:, :, 0]) and np.array_equal(ext[:, :, 4], other[:, :, 4])      # (H itself does not depend on it)
