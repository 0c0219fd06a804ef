"""tests/catalog_ref.py held to hand-worked cases, and tests/catalog_cases.py shown - from the reference alone - not to be degenerate: what the
GPU tests compare on these cases is worth comparing."""
import numpy as np
import pytest

from tests import catalog_cases as cc
from tests import catalog_ref as cref
from tests import flank_ref as fref
from tests import motif_search_ref as ref


def _codes(s):
    return np.array(["ACGT".index(c) for c in s], np.uint8)


def test_hand_worked_seeds_and_candidates():
    A, M, B = _codes("ACGTACGGTTCAGGCA"), _codes("CAG"), _codes("TTGACCGATAGGCTAA")
    assert cref.seeds(A, 1, 8) == [tuple(_codes("ACGTACGG")), tuple(_codes("TTCAGGCA"))]
    with pytest.raises(AssertionError):
        cref.seeds(A, 2, 8)
    x = np.concatenate([_codes("GG"), A, np.tile(M, 4), B, _codes("T")])
    reads = [x, ref.revcomp(x), np.concatenate([A, np.tile(M, 4)]), np.concatenate([A, ref.revcomp(B)]), _codes("ACGTACG")]
    loci = [(A, M, B)]
    assert cref.candidates(reads, loci, 1, 8) == [(0, 0, 0), (1, 0, 1)]                 # one side only, and A with rc B, are no candidates
    rows, cands = cref.genotype(reads, loci, 1, 8)
    assert [(r[0], r[1], r[2], r[3], r[4]) for r in rows] == [(0, 0, 0, (0, 0), (18, 30)), (1, 0, 1, (0, 0), (17, 29))]
    assert rows[0][5] == (18, 29, 12, 4, 12, 0, 0, 0) and rows[0][6] == 12 and rows[0][7] == np.float32(1)
    dense, _ = fref.genotype(reads, loci, 1)
    assert dense[0][:, 0].tolist() == [1, 1, 0, 0, 0]
    # one substitution in the first seed: still a candidate through the second seed, and spanning at K = 1; at K = 0 with q = 16 it is neither
    y = x.copy()
    y[2 + 3] = (y[2 + 3] + 1) & 3
    assert cref.candidates([y], loci, 1, 8) == [(0, 0, 0)] and cref.genotype([y], loci, 1, 8)[0][0][3] == (1, 0)
    assert cref.candidates([y], loci, 0, 16) == [] and fref.genotype([y], loci, 0)[0][0][0, 0] == 0


@pytest.mark.parametrize("K,q", cc.KQ)
def test_the_rows_are_the_dense_definition_s_spanning_rows(K, q):
    """the pigeonhole argument, checked: dropping the non-candidates loses no spanning pair (on the first loci, where the dense reference is cheap)"""
    loci, reads = cc.cases(K, q)
    loci = loci[:8]
    rows, _ = cref.genotype(reads, loci, K, q)
    (sp, o, fd, w, f, sc, ra), _ = fref.genotype(reads, loci, K)
    assert [(r[0], r[1]) for r in rows] == [tuple(int(v) for v in at) for at in np.argwhere(sp == 1)]
    for r, l, ori, dist, win, fields, score, ratio in rows:
        assert (int(o[r, l]), tuple(fd[r, l]), tuple(w[r, l]), tuple(f[r, l]), int(sc[r, l]), ra[r, l]) == (ori, dist, win, fields, score, ratio), (r, l)


@pytest.mark.parametrize("K,q", cc.KQ)
def test_the_cases_are_not_degenerate(K, q):
    loci, reads = cc.cases(K, q)
    need = (K + 1) * q
    rows, cands = cref.genotype(reads, loci, K, q)
    span = {(r[0], r[1]): r for r in rows}
    sets = [cref.qmers(x, q) for x in reads]
    hits = cref.read_hits(reads, loci, K, q)
    # every seed index is the only surviving seed of the left pattern of some spanning row
    alone = set()
    for (r, l), row in span.items():
        got = cref.seeded(sets[r], cref.slots(loci[l])[2 * row[2]], K, q)
        if len(got) == 1:
            alone.add(got[0])
    assert alone == set(range(K + 1)), alone
    flank_lens = {len(p) for A, _, B in loci for p in (A, B)}
    assert {need, min(need + 1, 64), 64} <= flank_lens
    # candidates that do not span; reads seeded on one side only; A in one orientation and B in the other
    idle = [(r, l) for r, l, _ in cands if (r, l) not in span]
    assert len(idle) >= 3
    one_side = [r for r, got in enumerate(hits) if got and not any(c[0] == r for c in cands)]
    assert len(one_side) >= 3
    assert any((1, 0) in got and (1, 3) in got and (1, 1) not in got and (1, 2) not in got for got in hits)
    # both orientations candidates and valid: a tie (orientation 0) and, with K > 0, the reverse one nearer
    both = [(r, l) for r, l, o in cands if o == 1 and (r, l, 0) in set(cands) and (r, l) in span]
    assert any(span[p][2] == 0 for p in both) and (K == 0 or any(span[p][2] == 1 for p in both))
    assert loci[6][0] is loci[1][0] or np.array_equal(loci[6][0], loci[1][0])          # two loci share a flank
    per_read = [len({l for r, l, _ in cands if r == i}) for i in range(len(reads))]
    assert max(per_read) >= cc.MANY
    rep = tuple([0, 1] * (q // 2))
    assert max(sum(tuple(int(c) for c in x[p:p + q]) == rep for p in range(len(x) - q + 1)) for x in reads) >= 20
    assert any(row[4][0] == row[4][1] for row in rows)                                 # an empty window
    U = {len(loci[l][1]) for (_, l) in span}
    assert min(U) <= 16 and max(U) >= 17                                               # both sides of the lane / wave border
    assert sum(row[2] == 0 for row in rows) >= 20 and sum(row[2] == 1 for row in rows) >= 15


def test_the_count_cases_have_one_candidate_and_one_row_a_read():
    loci, reads = cc.count_cases(257)
    rows, cands = cref.genotype(reads, loci, 2, 12)
    assert [c[0] for c in cands] == list(range(257)) and [r[0] for r in rows] == list(range(257))


def test_the_big_catalogue_s_other_loci_have_no_seed_in_any_read():
    """so they provably have no row: the GPU test compares with the dense call on the carried loci and twenty others only"""
    A, motifs, B, reads, carried = cc.big_catalog()
    K, q = cc.BIG_K, cc.BIG_Q
    other = np.setdiff1d(np.arange(cc.BIG_LOCI), carried)
    seeds = []
    for F in (A[other], B[other]):
        for P in (F, (3 - F)[:, ::-1]):
            seeds.append(cc.codes_of(P, q)[:, [i * q for i in range(K + 1)]].ravel())
    seeds = np.unique(np.concatenate(seeds))
    held = np.unique(np.concatenate([cc.codes_of(x[None, :], q).ravel() for x in reads]))
    assert not np.isin(held, seeds).any()
    assert len(carried) == cc.BIG_CARRIED and max(len(x) for x in reads) <= 400
