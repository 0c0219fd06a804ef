"""The allele calls' reference (tests/allele_call_ref.py) against hand-worked lists, and the inputs of tests/allele_call_cases.py shown not to be
degenerate from the reference alone (CPU): what tests/test_gpu_allele_call.py compares the library with is worth comparing with."""
import numpy as np
import pytest

from tests import allele_call_cases as cases
from tests import allele_call_ref as aref
from tests import flank_ref as fref


def _split(v, rule=(3, 20, 2)):
    z, call, sup, cost, k, why = aref.split(np.sort(np.array(v, np.int64)), *rule)
    return z, call, sup, cost, k, why


def test_the_four_examples_of_the_definition():
    z, call, sup, cost, k, _ = _split([19, 20, 20, 20, 20, 21, 34, 35, 35, 35, 36])
    assert (z, call, sup, cost, k) == (2, (20, 35), (6, 5), (76, 4), 6)
    # by hand: the median of all eleven is 21 -> 2 + 1 * 4 + 0 + 13 + 14 * 3 + 15 = 76; the halves: 1 + 0 + 1 = 2 and 1 + 0 + 1 = 2
    z, call, sup, cost, k, _ = _split([10] * 9 + [40])
    assert (z, call, sup, cost, k) == (1, (10, 10), (10, 0), (30, 30), 0)        # one read is neither 3 reads nor 20 %
    z, call, sup, cost, k, why = _split([10, 10, 10, 40, 40, 40, 70, 70, 70])
    assert (z, call, sup, cost, k) == (2, (10, 40), (3, 6), (180, 90), 3) and why["tie"]      # k = 3 and k = 6 both cost 90: the smaller k
    z, call, sup, cost, k, _ = _split([0, 0, 0, 0, 12, 12, 13])
    assert (z, call, sup, cost, k) == (2, (0, 12), (4, 3), (37, 1), 4)


def test_no_one_and_two_supporting_reads_and_all_values_equal():
    assert _split([])[:5] == (0, (0, 0), (0, 0), (0, 0), 0)
    assert _split([5])[:5] == (0, (0, 0), (0, 0), (0, 0), 0)
    assert _split([5], (1, 0, 1))[:5] == (1, (5, 5), (1, 0), (0, 0), 0)
    assert _split([4, 9], (1, 0, 1))[:5] == (2, (4, 9), (1, 1), (5, 0), 1)
    assert _split([4, 9], (2, 0, 1))[:5] == (1, (4, 4), (2, 0), (5, 5), 0)        # the lower median of two
    assert _split([4, 9], (3, 0, 1))[:5] == (0, (0, 0), (0, 0), (0, 0), 0)
    assert _split([7] * 6, (1, 0, 1))[:5] == (1, (7, 7), (6, 0), (0, 0), 0)
    # each condition alone refuses a split
    assert _split([5, 5, 9, 9, 9])[5]["support"] == 1 and _split([1, 1, 2, 2], (2, 50, 5))[5]["sep"] == 1
    assert _split([10] * 9 + [40], (1, 20, 2))[5]["percent"] == 1 and _split([1, 5, 5, 9], (1, 0, 1))[5]["distinct"] == 1


def test_the_columns_of_a_small_input():
    rows = cases.from_lists([[9, 4, 4], [], [3]])
    (off, value, read, allele, zyg, call, sup, cost), _ = aref.call_alleles(rows, 0, cases.MIN_RATIO, 1, 0, 1)
    assert off.tolist() == [0, 3, 3, 4] and value.tolist() == [4, 4, 9, 3] and allele.tolist() == [0, 0, 1, 0] and zyg.tolist() == [2, 0, 1]
    assert read[0] < read[1] and call.tolist() == [[4, 9], [0, 0], [3, 3]] and sup.tolist() == [[2, 1], [0, 0], [1, 0]] and cost.tolist() == [[5, 0], [0, 0], [0, 0]]
    assert (off.dtype, value.dtype, read.dtype, allele.dtype, zyg.dtype, call.dtype, sup.dtype, cost.dtype) == (
        np.int64, np.int32, np.int32, np.uint8, np.uint8, np.int32, np.int32, np.int64)
    bases = aref.call_alleles(rows, 1, cases.MIN_RATIO, 1, 0, 1)[0]
    assert bases[1].tolist() == [12, 12, 27, 9]
    # the dropped rows hold negative values: with min_ratio = 0 they support, and that is an error naming the row
    with pytest.raises(ValueError, match="row "):
        for seed in range(20):
            aref.call_alleles(cases.from_lists([[9, 4, 4]], seed), 0, 0.0, 1, 0, 1)


@pytest.fixture(scope="module")
def everything():
    """the reference on every built input under every rule of the sweep, measure copies and bases: [(name, measure, rule, columns, whys)]"""
    inputs = [("tile_edges", cases.tile_edges()), ("many_loci", cases.many_loci()), ("hand", cases.from_lists())] + [
        (f"lane_edges_{m}", cases.lane_edges(m)) for m in (63, 64, 65)]
    out = []
    for name, rows in inputs:
        for measure in (0, 1):
            for rule in cases.SWEEP:
                out.append((name, measure, rule) + aref.call_alleles(rows, measure, cases.MIN_RATIO, *rule))
    return out


def test_the_built_inputs_are_not_degenerate(everything):
    zyg = np.concatenate([c[4] for _, _, _, c, _ in everything])
    assert {0, 1, 2} == set(zyg.tolist()) and min((zyg == z).sum() for z in (0, 1, 2)) >= 10
    whys = [w for *_, ws in everything for w in ws]
    assert any(w["tie"] for w in whys)
    for cond in aref.CONDITIONS:
        assert sum(w[cond] for w in whys) >= 1, cond
    edge = {(measure, rule): c for name, measure, rule, c, _ in everything if name == "tile_edges"}
    for (measure, rule), c in edge.items():
        assert np.diff(c[0]).tolist() == list(cases.EDGE_SUPPORT), (measure, rule)
    # the last edge locus under bases: cost1, and the sum of its values, pass 2^31
    big = edge[(1, cases.SWEEP[1])]
    assert big[7][-1, 0] > 2 ** 31 and big[1][big[0][-2]:].astype(np.int64).sum() > 2 ** 31 and big[4][-1] == 2 and big[7][-1, 1] < 2 ** 31
    # equal values keep the read order; descending values come out reversed
    off, value, read = edge[(0, cases.SWEEP[0])][:3]
    for l, kind in enumerate(cases.KINDS * 4):
        rd, v = read[off[l]:off[l + 1]], value[off[l]:off[l + 1]]
        assert (np.diff(v) >= 0).all() and ((np.diff(v) > 0) | (np.diff(rd) > 0)).all()
        if kind == "descending" and len(rd) > 1:
            assert (np.diff(rd) < 0).all()
    many = next(c for name, measure, rule, c, _ in everything if name == "many_loci")
    assert (np.diff(many[0]) == 0).mean() > 0.5 and many[0][1] == 0 and many[0][-1] > many[0][-2]


def test_rows_dropped_by_the_ratio_and_empty_windows_kept():
    rows = cases.tile_edges()
    kept, _ = aref.supporting(*rows, 0, cases.MIN_RATIO)
    assert ((rows.spanning == 1) & ~kept).sum() >= 1000 and (rows.ratio[kept] == np.float32(cases.MIN_RATIO)).sum() >= 100
    assert (rows.ratio[(rows.spanning == 1) & ~kept] == np.nextafter(np.float32(cases.MIN_RATIO), np.float32(0))).sum() >= 100
    assert ((rows.spanning == 0) & ((rows.fields[:, :, 3] < 0) | np.isnan(rows.ratio))).sum() >= 1000          # garbage where nothing spans
    (off, value, read, *_), _ = aref.call_alleles(cases.empty_windows(), 0, 1.0, 2, 20, 1)
    assert value.tolist() == [0, 0, 0, 6] and read.tolist() == [0, 2, 3, 1]


def test_end_to_end_on_the_reference():
    """the committed seed: flank_ref.genotype, then the reference, gives the alleles the reads were built with"""
    reads, loci = cases.e2e()
    assert len(reads) == 26
    cols, _ = fref.genotype(reads, loci, cases.E2E_K)
    gt = cases.Rows(cols[0], cols[3], cols[4], cols[6])
    (off, value, read, allele, zyg, call, sup, cost), _ = aref.call_alleles(gt, 0, cases.E2E_MIN_RATIO, *cases.E2E_RULE)
    assert zyg.tolist() == [2, 1] and call.tolist() == [[5, 12], [8, 8]] and sup.tolist() == [[9, 7], [6, 0]]
    assert np.diff(off).tolist() == [16, 6] and allele.tolist() == [0] * 9 + [1] * 7 + [0] * 6
    rule = cases.E2E_RULE[:2] + (6,)
    (_, _, _, _, zyg, call, sup, _), _ = aref.call_alleles(gt, 1, cases.E2E_MIN_RATIO, *rule)
    assert zyg.tolist() == [2, 1] and call.tolist() == [[15, 36], [48, 48]] and sup.tolist() == [[9, 7], [6, 0]]
