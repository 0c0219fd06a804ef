"""tests/partial_catalog_ref.py - the partial genotype at catalogue scale as include/mtr_hip.h defines it - against the dense definition
(tests/partial_ref.py) on the inputs of tests/partial_catalog_cases.py: its rows are the dense reference's partial rows, every column; and the
inputs are not degenerate, shown from the references alone.  CPU only."""
import functools

import numpy as np
import pytest

from tests import catalog_cases as cc
from tests import catalog_ref as cref
from tests import flank_ref as fref
from tests import partial_cases as pc
from tests import partial_catalog_cases as pcc
from tests import partial_catalog_ref as pcr
from tests import partial_ref as pref

MIXED = [(5, 8, 130), (17, 32, 70)]


@functools.lru_cache(maxsize=None)
def _sparse(kind, K, q, priority=pref.SUB_LEFT_UP):
    loci, reads = _inputs(kind)
    return pcr.genotype_partial_catalog(reads, loci, K, q, max_tail=pcc.MAX_TAIL, priority=priority)


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    if kind == "grid":
        return pc.LOCI, pc.BATCH
    if kind[0] == "cases":
        return pcc.cases(*kind[1:])
    if kind[0] == "mixed":
        return pcc.mixed(*kind[1:])[:2]
    return pcc.count_cases(kind[1])


def _same(rows, dense):
    assert len(rows) == len(dense), (len(rows), len(dense))
    for a, b in zip(rows, dense):
        assert a[:6] == b[:6] and a[7] == b[7] and np.float32(a[6]).tobytes() == np.float32(b[6]).tobytes(), (a, b)


@pytest.mark.parametrize("K,q", pcc.GRID_KQ)
def test_the_grid_s_rows_are_the_dense_reference_s_and_the_counts_are_the_known_ones(K, q):
    rows, cands = _sparse("grid", K, q)
    _same(rows, pcr.dense_rows(pc.want(K) if K in pc.KS else pref.genotype_partial(pc.BATCH, pc.LOCI, K, max_tail=pc.MAX_TAIL)))
    assert (len(cands), len(rows)) == pcc.GRID_COUNTS[(K, q)]
    assert all(rows[i][:2] < rows[i + 1][:2] for i in range(len(rows) - 1))


@pytest.mark.parametrize("K,q", pcc.KQ)
def test_the_new_set_s_rows_are_the_dense_reference_s_and_it_is_not_degenerate(K, q):
    loci, reads = _inputs(("cases", K, q))
    rows, cands = _sparse(("cases", K, q), K, q)
    _same(rows, pcr.dense_rows(pref.genotype_partial(reads, loci, K, max_tail=pcc.MAX_TAIL)))
    assert sorted({len(A) for A, _, B in loci} | {len(B) for A, _, B in loci}) == sorted({(K + 1) * q, min((K + 1) * q + 1, 64), 64})
    found = pcr.seeded_hits(reads, loci, cands)
    is_row = {r[:2] for r in rows}
    four = {(r, l): pcr.four_hits(found, r, l, mask, K) for r, l, mask in cands}
    spanning = [c for c in cands if fref.pair(*four[c[:2]], K)[0]]
    beyond = [c for c in cands if bin(c[2]).count("1") == 1 and min(f[0] for f in four[c[:2]]) > K]
    assert len(spanning) >= 16 + pcc.MANY and len(beyond) >= 1 and not {c[:2] for c in spanning + beyond} & is_row
    # every slot chosen for every bucket, at both of the bucket's edges
    assert {(len(loci[r[1]][1]), r[2]) for r in rows} >= {(U, s) for U in pcc.US for s in range(4)}
    masks = {c[:2]: c[2] for c in cands}
    assert any(bin(masks[r[:2]]).count("1") > 1 for r in rows)                                          # the chosen slot is not the only seeded one
    ties = [r for r in rows if sum(1 for f in four[r[:2]] if f[0] == r[3]) > 1]
    assert {r[2] for r in ties} >= {0, 2}                                                               # a tie goes to the lowest slot
    assert any(r[2] == 3 and four[r[:2]][0][0] <= K for r in rows)                                      # a higher slot wins by distance
    per_read = {}
    for r, l, _ in cands:
        per_read[r] = per_read.get(r, 0) + 1
    assert max(per_read.values()) >= 64
    assert sum(1 for r in rows if r[4][0] == r[4][1]) >= 3                                              # empty windows
    assert sum(1 for r in rows if r[4][1] > r[4][0] and r[5][0] == 0) >= 2                              # windows without a positive cell
    assert {r[3] for r in rows} >= {0, K}


@pytest.mark.parametrize("first_u,last_u,n", MIXED)
def test_every_lane_of_the_mixed_wavefronts_has_its_own_motif_length_and_direction(first_u, last_u, n):
    loci, reads, what = pcc.mixed(first_u, last_u, n)
    rows, cands = _sparse(("mixed", first_u, last_u, n), 0, 12)
    _same(rows, pcr.dense_rows(pref.genotype_partial(reads, loci, 0, max_tail=pcc.MAX_TAIL)))
    assert len(rows) == n and [(r[0], r[1], r[2], r[4][1] - r[4][0]) for r in rows] == [(i, l, s, wl) for i, (l, s, wl) in enumerate(what)]
    assert [r[2] for r in rows] == [i % 4 for i in range(n)]
    assert len({tuple(m.tolist()) for _, m, _ in loci}) == n and {len(m) for _, m, _ in loci} == set(range(first_u, last_u + 1))
    assert {r[4][0] % 16 for r in rows if r[2] in (0, 3)} == set(range(16)) and {r[4][1] % 16 for r in rows if r[2] in (1, 2)} == set(range(16))
    lens = [r[4][1] - r[4][0] for r in rows]
    assert min(lens) == 7 and max(lens) == 110 and all(r[5][0] > 0 for r in rows)
    # the predecessor rule shows in motif_bases or matches in every stretch of 64 rows, the last, partial one included: the wavefronts of the launch
    # where the tasks are appended in the candidates' order (a wavefront takes 64 consecutive tasks of the bucket's list)
    other, _ = _sparse(("mixed", first_u, last_u, n), 0, 12, pref.UP_LEFT_SUB)
    moved = [a[5][1] != b[5][1] or a[5][3] != b[5][3] for a, b in zip(rows, other)]
    print(sum(moved), "of", n, "rows depend on the predecessor's order")
    assert n % 64 and all(any(moved[w:w + 64]) for w in range(0, n, 64))


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_the_count_cases_have_exactly_that_many_rows(count):
    loci, reads = _inputs(("count", 257))
    rows, cands = pcr.genotype_partial_catalog(reads[:count], loci, 2, 12, max_tail=pcc.MAX_TAIL) if count < 257 else _sparse(("count", 257), 2, 12)
    assert len(rows) == len(cands) == count and [r[0] for r in rows] == list(range(count))
    assert all(r[4][1] > r[4][0] for r in rows)
    if count == 257:
        _same(rows, pcr.dense_rows(pref.genotype_partial(reads, loci, 2, max_tail=pcc.MAX_TAIL)))
        assert {r[2] for r in rows} == {0, 1, 2, 3} and {r[1] for r in rows} == {0, 1}


def test_no_cut_read_of_the_big_catalogue_holds_a_seed_of_a_locus_it_does_not_carry():
    A, motifs, B, reads, carried = pcc.big_cut()
    K, q = cc.BIG_K, cc.BIG_Q
    assert max(len(r) for r in reads) <= 400 and len(reads) == cc.BIG_READS
    held = np.unique(np.concatenate([cc.codes_of(x[None, :], q).ravel() for x in reads]))
    at = [i * q for i in range(K + 1)]
    hit = np.zeros(cc.BIG_LOCI, bool)
    for F in (A, B):
        for P in (F, (3 - F)[:, ::-1]):
            hit |= np.isin(cc.codes_of(P, q)[:, at], held).any(axis=1)
    assert sorted(np.nonzero(hit)[0].tolist()) == carried
    # on the carried loci every cut read is one partial row, of its own locus, with a window of at least a copy, and spans nothing
    loci = [(A[l], motifs[l], B[l]) for l in carried]
    rows, cands = pcr.genotype_partial_catalog(reads, loci, K, q)
    assert len(cands) >= len(rows) == len(reads) and [r[0] for r in rows] == list(range(len(reads)))      # (a carried locus' chance seed: a candidate, no row)
    assert [r[1] for r in rows] == [i % cc.BIG_CARRIED for i in range(len(reads))]
    assert {r[2] for r in rows} == {0, 1, 2, 3} and all(r[4][1] - r[4][0] >= 4 for r in rows)
    assert cref.candidates(reads, loci, K, q) == []                                                     # none holds both flanks of an orientation
