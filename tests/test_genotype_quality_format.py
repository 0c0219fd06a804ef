"""mtr_amd.format_genotype_quality and mtr_amd.with_reassigned_alleles on CPU tensors and numpy (no GPU, no library): the formatter's lines, and
the reassignment on a locus that moves two entries, one where a side would empty, and one of zygosity 1."""
import numpy as np
import pytest

import mtr_amd

torch = pytest.importorskip("torch")

LOCI = [("ACGT", "CAG", "TTGA"), ("GGAT", "GAA", "CCAT"), ("AAAC", "CGG", "TGCA"), ("CCCA", "AT", "GGGT")]


def _calls():
    """locus 0: zygosity 2, values 10 11 12 | 20 21; locus 1: zygosity 2, 5 6 | 9; locus 2: zygosity 1, 7 8 8; locus 3: no support"""
    t = torch.tensor
    return mtr_amd.AlleleCalls(t([0, 5, 8, 11, 11]), t([10, 11, 12, 20, 21, 5, 6, 9, 7, 8, 8], dtype=torch.int32), t([3, 1, 4, 0, 2, 1, 2, 0, 0, 1, 2], dtype=torch.int32),
                               t([0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0], dtype=torch.uint8), t([2, 2, 1, 0], dtype=torch.uint8),
                               t([[11, 20], [5, 9], [8, 8], [0, 0]], dtype=torch.int32), t([[3, 2], [2, 1], [3, 0], [0, 0]], dtype=torch.int32),
                               t([[22, 3], [7, 1], [1, 1], [0, 0]]))


def _gq(best):
    t = torch.tensor
    S = len(best)
    return mtr_amd.GenotypeQuality(torch.zeros(S, 2, dtype=torch.int32), t(best, dtype=torch.uint8), torch.zeros(S, dtype=torch.int32),
                                   t([[40, 0, 55], [0, 3, 9], [12, -1, -1], [-1, -1, -1]]), t([[40, 0, 55], [0, 3, 9], [0, -1, -1], [-1, -1, -1]]),
                                   t([1, 0, 0, 255], dtype=torch.uint8), t([40, 3, -1, -1]), t([5, 2, 3, 0], dtype=torch.int32), t([0, 1, 0, 0], dtype=torch.int32))


def test_the_lines_are_the_calls_lines_and_four_columns_more():
    calls, gq = _calls(), _gq([0] * 11)
    lines = mtr_amd.format_genotype_quality(LOCI, calls, gq).decode().splitlines()
    base = mtr_amd.format_allele_calls(LOCI, calls).decode().splitlines()
    assert [l.split("\t")[:-4] for l in lines] == [b.split("\t") for b in base]
    assert [l.split("\t")[-4:] for l in lines] == [["0/1", "40", "40,0,55", "5/0"], ["0/0", "3", "0,3,9", "2/1"], ["0/0", "-1", "0,-1,-1", "3/0"], ["./.", "-1", "-1,-1,-1", "0/0"]]
    as_numpy = mtr_amd.GenotypeQuality(*[x.numpy() for x in gq])
    assert mtr_amd.format_genotype_quality(LOCI, mtr_amd.AlleleCalls(*[x.numpy() for x in calls]), as_numpy).decode().splitlines() == lines
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.format_genotype_quality(LOCI[:3], calls, gq)


def test_reassignment_moves_entries_keeps_a_side_from_emptying_and_leaves_one_allele_alone():
    calls = _calls()
    # locus 0: the entry of value 12 goes to allele 1 and the one of value 20 to allele 0; locus 1: every entry would go to allele 1; locus 2: zygosity 1
    got = mtr_amd.with_reassigned_alleles(calls, _gq([0, 0, 1, 0, 1, 1, 1, 1, 1, 0, 1]))
    assert got.value.tolist() == [10, 11, 20, 12, 21, 5, 6, 9, 7, 8, 8] and got.read.tolist() == [3, 1, 0, 4, 2, 1, 2, 0, 0, 1, 2]
    assert got.allele.tolist() == [0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0]
    assert got.call.tolist() == [[11, 12], [5, 9], [8, 8], [0, 0]] and got.call_support.tolist() == [[3, 2], [2, 1], [3, 0], [0, 0]]
    assert torch.equal(got.cost, calls.cost) and torch.equal(got.support_off, calls.support_off) and torch.equal(got.zygosity, calls.zygosity)
    assert [x.dtype for x in got] == [x.dtype for x in calls] and [x.shape for x in got] == [x.shape for x in calls]
    # an uneven move: one entry of locus 0 to allele 1, one of locus 1 to allele 1
    got = mtr_amd.with_reassigned_alleles(calls, _gq([0, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0]))
    assert got.value.tolist() == [10, 12, 11, 20, 21, 5, 6, 9, 7, 8, 8] and got.allele.tolist() == [0, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0]
    assert got.call.tolist() == [[10, 20], [5, 6], [8, 8], [0, 0]] and got.call_support.tolist() == [[2, 3], [1, 2], [3, 0], [0, 0]]
    # nothing to move: the calls as they are
    same = mtr_amd.with_reassigned_alleles(calls, _gq(calls.allele.tolist()))
    assert all(torch.equal(x, y) for x, y in zip(same, calls))
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.with_reassigned_alleles(calls, _gq([0] * 10))
