"""The definition of the known-motif search (tests/motif_search_ref.py, the Python form of include/mtr_hip.h's) against the CPU oracle:
it equals Oracle.wrap_dp on the read shifted by one base - window 0 .. L - 1 of [a base] + x - with rep_start and rep_end each lowered by
one; a read without a positive cell maps to (0, -1, 0, 0, 0, 0, 0, 0); and score == G * matches - MM * mismatches - D * (insertions +
deletions).  These three facts are what the GPU tests take their truth from."""
import numpy as np
import pytest

from tests import motif_search_ref as ref
from tests.oracle_binding import Oracle

US = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33)
SCORES = ref.SCORE_SETS + [(1, 1, 1)]


@pytest.fixture(scope="module")
def orc():
    o = Oracle()
    yield o
    o.close()


def _lengths(U):
    return sorted({1, 2, 3, U, U + 1, 40, 97})


@pytest.mark.parametrize("U", US)
def test_the_definition_is_the_oracle_on_the_shifted_read(orc, U):
    rng = np.random.RandomState(1000 + U)
    motifs = [rng.randint(0, 4, size=U).astype(np.uint8), rng.randint(0, 2, size=U).astype(np.uint8)]
    n = hits = 0
    for m in motifs:
        for L in _lengths(U):
            for kind in ref.KINDS:
                x = ref.make_read(rng, kind, L, m)
                for G, MM, D in SCORES:
                    got = ref.align(x, m, G, MM, D)
                    w = orc.wrap_dp(np.concatenate([np.zeros(1, np.uint8), x]), 0, L - 1, m, G, MM, D)
                    assert got[:8] == (w[0] - 1, w[1] - 1) + tuple(w[2:]), (U, L, kind, (G, MM, D), x.tolist(), m.tolist())
                    assert got[8] == G * got[4] - MM * got[5] - D * (got[6] + got[7])
                    assert got == ref.oracle_align(orc)(x, m, G, MM, D)
                    if got[8] == 0:
                        assert got[:8] == ref.NO_HIT
                    else:
                        assert 0 <= got[0] <= got[1] < L and got[2] == got[1] - got[0] + 1 == got[4] + got[5] + got[6]
                    n += 1
                    hits += got[8] > 0
    assert n == 2 * len(_lengths(U)) * 4 * 4 and hits > n // 3


def test_of_two_equal_runs_the_first_wins(orc):
    """20 clean bases, 110 bases the motif does not hold, the same 20 again: bridging the junk costs more than a run gains under every score set,
    so the two runs are two equal maxima and the first in row-major order is the hit"""
    for U in (2, 3, 5, 8):
        m = np.arange(U, dtype=np.uint8) % 3                    # holds no T
        run = np.array([m[i % U] for i in range(20)], np.uint8)
        x = np.concatenate([run, np.full(110, 3, np.uint8), run])
        for G, MM, D in SCORES:
            got = ref.align(x, m, G, MM, D)
            assert got == (0, 19, 20, 20 // U, 20, 0, 0, 0, 20 * G), (U, got)
            assert got == ref.oracle_align(orc)(x, m, G, MM, D)


def test_a_read_without_the_motifs_bases_has_no_hit(orc):
    m = ref.codes_of("CAG")
    x = np.full(40, 3, np.uint8)
    for G, MM, D in SCORES:
        assert ref.align(x, m, G, MM, D) == ref.NO_HIT + (0,) == ref.oracle_align(orc)(x, m, G, MM, D)


def test_strands():
    m = ref.codes_of("CAG")
    x = np.tile(ref.revcomp(m), 12)
    (got, strand) = ref.search(x, m, 1, 1, 1)
    assert strand == 1 and got == ref.align(x, ref.revcomp(m), 1, 1, 1) and got[:4] == (0, 35, 36, 12)
    assert ref.search(x, m, 1, 1, 1, both_strands=False)[1] == 0
    for pal in ("AT", "ACGT"):
        p = ref.codes_of(pal)
        assert (ref.revcomp(p) == p).all()
        assert ref.search(np.tile(p, 9), p, 1, 1, 1)[1] == 0
    assert ref.search(np.tile(ref.codes_of("ACAC"), 5), ref.codes_of("ACAC"), 1, 1, 1)[0][3] == 5     # as given: copies of four bases
