"""The definition of the known-motif locus search (tests/motif_loci_ref.py, the Python form of include/mtr_hip.h's recursion) on the CPU: it
gives the same loci over the plain-Python aligner and over the CPU oracle (what the GPU tests take their truth from); with one round it is the
known-motif search filtered by the threshold; loci ascend and never overlap; `open` is set exactly when the recursion met depth R on a window
that could hold a locus; and the crafted three-tract read has its three tracts on strands 0, 1, 0."""
import numpy as np
import pytest

from tests import motif_loci_ref as lref
from tests import motif_search_ref as ref
from tests.oracle_binding import Oracle

SCORES = ref.SCORE_SETS


@pytest.fixture(scope="module")
def orc():
    o = Oracle()
    yield o
    o.close()


def _cases():
    """(read, motif, scores, S): 48 reads of at most 200 bases, every kind, the three score sets"""
    rng = np.random.RandomState(4242)
    motifs = [ref.codes_of(s) for s in ("CAG", "AT", "A", "AACCCT")] + [rng.randint(0, 3, size=u).astype(np.uint8) for u in (5, 17)]
    out = []
    for k in range(48):
        m = motifs[k % len(motifs)]
        L = (1, 2, 200, 199)[k] if k < 4 else int(rng.randint(3, 201))
        G, MM, D = SCORES[k % 3]
        out.append((ref.make_read(rng, ref.KINDS[k % 4], L, m), m, (G, MM, D), G * (4 + k % 9)))
    return out


CASES = _cases()


def _well_formed(got, L):
    prev_end = -1
    for hit, strand in got:
        assert strand in (0, 1) and prev_end < hit[0] <= hit[1] < L and hit[2] == hit[1] - hit[0] + 1 >= 1, got
        prev_end = hit[1]


def test_the_recursion_is_the_same_over_the_python_aligner_and_the_oracle(orc):
    one = ref.oracle_align(orc)
    total = several = opened = 0
    for x, m, sc, S in CASES:
        for R in (1, 2, 16):
            for both in (True, False):
                a, b = lref.loci(x, m, *sc, S, R, both), lref.loci(x, m, *sc, S, R, both, one=one)
                assert a == b, (x.tolist(), m.tolist(), sc, S, R, both)
                _well_formed(a[0], len(x))
                assert all(h[8] >= S for h, _ in a[0])
                total += len(a[0]); several += len(a[0]) > 1; opened += a[1]
    assert total > 200 and several > 30 and opened > 10


def test_one_round_is_the_search_filtered_by_the_threshold():
    kept = 0
    for x, m, sc, S in CASES:
        hit, strand = ref.search(x, m, *sc)
        got, _ = lref.loci(x, m, *sc, S, 1)
        assert got == ([(hit, strand)] if hit[8] >= S else [])
        kept += len(got)
    assert 10 < kept < len(CASES)


def _open_by_hand(x, m, sc, S, R):
    """the flag without the recursion's own bookkeeping: run it unbounded and remember the depth of every window of at least minlen bases"""
    ml, deep = lref.minlen(S, sc[0]), []

    def rec(lo, hi, depth):
        if hi - lo < ml:
            return
        deep.append(depth)
        hit, _ = ref.search(x[lo:hi], m, *sc)
        if hit[8] >= S:
            rec(lo, lo + hit[0], depth + 1); rec(lo + hit[1] + 1, hi, depth + 1)
    rec(0, len(x), 0)
    return int(max(deep, default=0) >= R)


def test_open_is_set_exactly_when_a_window_stands_at_depth_R():
    seen = set()
    for x, m, sc, S in CASES:
        for R in (1, 2, 3):
            want = _open_by_hand(x, m, sc, S, R)
            assert lref.loci(x, m, *sc, S, R)[1] == want
            seen.add(want)
        full, op = lref.loci(x, m, *sc, S, 32)
        if not op:                                                        # nothing left open: fewer rounds find a subset, in order
            part = lref.loci(x, m, *sc, S, 2)[0]
            assert [h for h in full if h in part] == part
    assert seen == {0, 1}


def test_the_three_tracts_of_the_crafted_read(orc):
    x, m = lref.three_tracts(), ref.codes_of("CAG")
    for one in (ref.align, ref.oracle_align(orc)):
        got, op = lref.loci(x, m, 1, 1, 1, 12, 16, one=one)
        assert len(got) >= 3 and op == 0
        _well_formed(got, len(x))
        big = [(h, s) for h, s in got if h[8] >= 18]
        assert [s for _, s in big] == [0, 1, 0], got
        assert big[0][0] == (23, 67, 45, 15, 45, 0, 0, 0, 45) and big[2][0][0] == 23 + 45 + 31 + 30 + 18 and big[1][0][8] >= 30
        assert 23 + 45 + 31 - 2 <= big[1][0][0] <= 23 + 45 + 31 and big[1][0][1] in range(23 + 45 + 31 + 29, 23 + 45 + 31 + 32)
        assert big[2][0][5] == 2                                          # the two substitutions, as mismatches
    assert lref.loci(x, m, 1, 1, 1, 12, 16, both_strands=False)[0][0][1] == 0
    assert len(lref.loci(x, m, 1, 1, 1, 12, 1)[0]) == 1
