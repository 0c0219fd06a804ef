"""The cases of tests/dp_pass_cases.py, held to the CPU oracle alone (no GPU): they are not degenerate.

  * every 16-bit limit case is a perfect repeat whose score really gets to the limit: matches == rows, no edits;
  * every base-absent case aligns nothing: an empty repeat (rep_start = qs + 1, rep_end = qs) and six zero counts;
  * on the small shapes (rows <= 41, U <= 33) the plain-Python definition of the DP (tests/motif_search_ref.align) gives the oracle's eight values;
  * among those small shapes enough hold their maximum in more than one cell, column and row: the best-cell rule (largest value, then smallest row,
    then smallest column) is exercised, not only its first clause.
"""
import numpy as np
import pytest

from tests import dp_pass_cases as dc
from tests import motif_search_ref as ms


@pytest.fixture(scope="module")
def orc():
    from tests.oracle_binding import Oracle
    o = Oracle()
    yield o
    o.close()


def _limit_cases():
    return dc.wave2p_limits() + dc.quad2p_limits() + dc.one_param_limits() + dc.entry_limits()


def test_limit_cases_reach_their_limit(orc):
    cases = _limit_cases()
    assert len(cases) >= 12 + 2 + 2 + 9 + 24
    for c in cases:
        sets = dc.SETS2 if c.tag.startswith(("WAVE2P", "QUAD2P")) else ((c.G, c.MM, c.D),)
        for p in sets:
            w = dc.oracle_want(orc, c, p)
            assert w == (c.qs + 1, c.qe + 1, c.rows, c.rows // c.U, c.rows, 0, 0, 0), (c, p, w)


def test_limit_rows_are_the_last_the_16_bit_passes_admit():
    for U in (2, 17, 128):
        for (G, MM, D) in dc.SETS3:
            r = dc.dpq_max_rows(U, G, D)
            assert 4 * (r * G + D * (U + 2)) < 65000 <= 4 * ((r + 1) * G + D * (U + 2))
    for U in (17, 128):
        assert dc.dpq_max_rows(U, 1, 3) == 16243 - 3 * U
    for U in (65, 128, 129, 256):
        for (G, MM, D) in dc.SETS3:
            r = dc.dpq_max_rows(U, G, D, 1)
            assert r * G + D * (U + 2) < 65000 <= (r + 1) * G + D * (U + 2)


def test_base_absent_cases_align_nothing(orc):
    cases = [c for c in dc.grid(dc.U64) + dc.small_grid() if c.kind == "absent"]
    assert len(cases) >= 40
    for c in cases:
        assert 3 not in set(int(v) for v in c.unit) and set(int(v) for v in c.read[c.qs + 1:c.qe + 2]) == {3}
        for p in dc.SETS3:
            assert dc.oracle_want(orc, c, p) == (c.qs + 1, c.qs, 0, 0, 0, 0, 0, 0), (c, p)


def test_placement_cases_sit_at_the_ends_of_their_reads(orc):
    """the window at the start of the first read begins with base 1 (qs = 0); the last row of the other is its read's last base, and the oracle aligns it"""
    for U in (16, 33, 49, 65, 129):
        first, last = dc.placement_cases(np.random.RandomState(77 + U), U)
        assert first.qs == 0 and len(first.read) > first.qe + 1
        assert last.qe + 1 == len(last.read) - 1
        for p in dc.SETS3:
            assert dc.oracle_want(orc, last, p)[1] == len(last.read) - 1, (U, p)           # the repeat ends on the read's last base
    ends = [c for c in dc.grid(dc.U64) if c.qe + 1 == len(c.read) - 1]
    assert len(ends) >= 30
    kinds = {(c.U, c.rows): c.kind for c in dc.grid(dc.U16, seed=12)}
    other = {(c.U, c.rows): c.kind for c in dc.grid(dc.U16, seed=14)}
    assert sum(1 for k in kinds if kinds[k] != other[k]) > len(kinds) // 2          # another pass, another kind at the same shape


def _definition(c):
    """the eight values from the plain-Python DP: row i is x[i - 1] there, base qs + i here"""
    a = ms.align(c.read[c.qs + 1:c.qe + 2], c.unit, c.G, c.MM, c.D)
    return (a[0] + c.qs + 1, a[1] + c.qs + 1) + tuple(a[2:8])


def _max_cells(c):
    """(cells, columns, rows) that hold the matrix's maximum (0 where nothing scores)"""
    x, m = [int(v) for v in c.read[c.qs + 1:c.qe + 2]], [int(v) for v in c.unit]
    U = len(m)
    H = np.zeros((len(x) + 1, U + 1), np.int64)
    for i in range(1, len(x) + 1):
        for j in range(1, U + 1):
            if x[i - 1] == m[j - 1]:
                v = H[i - 1, j - 1] + c.G
            else:
                v = max(0, H[i - 1, j - 1] - c.MM, H[i - 1, j] - c.D)
                if j > 1:
                    v = max(v, H[i, j - 1] - c.D)
            H[i, j] = v
        H[i, 0] = H[i, U]
    body = H[1:, 1:]
    if body.max() <= 0:
        return 0, 0, 0
    ii, jj = np.nonzero(body == body.max())
    return len(ii), len(set(jj.tolist())), len(set(ii.tolist()))


def test_small_shapes_match_the_definition_and_hold_ties(orc):
    cases = dc.small_grid()
    assert len(cases) >= 432 and all(c.rows <= 41 and c.U <= 33 for c in cases)
    bad = [(c, _definition(c), dc.oracle_want(orc, c)) for c in cases if _definition(c) != dc.oracle_want(orc, c)]
    assert not bad, f"{len(bad)} of {len(cases)} small shapes: definition and oracle differ, first {bad[0]}"
    tied = [_max_cells(c) for c in cases if c.kind in ("homopolymer", "ac", "two_runs", "random")]
    cells = sum(1 for t in tied if t[0] > 1)
    cols = sum(1 for t in tied if t[1] > 1)
    rows = sum(1 for t in tied if t[2] > 1)
    print(f"maximum in more than one cell / column / row: {cells} / {cols} / {rows} of {len(tied)}")
    assert cells >= 100 and cols >= 40 and rows >= 40, (cells, cols, rows, len(tied))
