"""The two kinds of catalogue call on one engine (mtr_genotype_catalog_device and mtr_genotype_partial_catalog_device, their prepared forms, their
copies and statistics): both run through one front and one tail and keep their rows in one kind of state, so each kind's kept rows and counts
must stay its own whichever call came last, a failed call must forget its own kind's rows alone, and an upload both.  Truth is the same call
alone on a fresh engine.  5 reads x 3 loci of tests/catalog_cases.py: a handful of tiny kernels."""
import pytest

import mtr_amd
from tests import catalog_cases as cc
from tests.test_gpu_catalog_prepared import _kept, _same, _texts

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

K, Q = 1, 8


def _cases():
    loci, reads = cc.cases(K, Q)
    # a spanning read of each of the loci 0, 1 and 2, and locus 1 seeded on the left only and on the right only
    return _texts(loci[:3]), [reads[2], reads[11], reads[20], reads[67], reads[68]]


@pytest.fixture(scope="module")
def alone():
    """each kind's rows and counts from its call alone on a fresh engine"""
    texts, reads = _cases()
    out = []
    for partial in (False, True):
        e = mtr_amd.Engine()
        try:
            e.upload(reads)
            rows = e.genotype_partial_catalog(texts, K, Q) if partial else e.genotype_catalog(texts, K, Q)
            counts = (e.test_partial_catalog_stats() if partial else e.test_catalog_stats())[0]
        finally:
            e.close()
        assert rows.read.numel() >= 2 and counts[3] == rows.candidates >= rows.read.numel()
        out.append((rows, counts))
    return out


def _both_kept(e, alone):
    """both kinds' copies and statistics, each against its call alone"""
    (sg, g_counts), (spg, p_counts) = alone
    m = len(_cases()[0])
    assert _same(e._catalog_rows(m, sg.read.numel(), sg.candidates), sg)
    assert _same(e._partial_catalog_rows(m, spg.read.numel(), spg.candidates), spg)
    assert e.test_catalog_stats()[0] == g_counts and e.test_partial_catalog_stats()[0] == p_counts
    assert _kept(e, False) and _kept(e, True)


def test_each_kind_keeps_its_own_rows_and_counts(alone):
    texts, reads = _cases()
    (sg, _), (spg, _) = alone
    e = mtr_amd.Engine()
    try:
        cat = e.build_catalog(texts, K, Q)
        e.upload(reads)
        text_calls = (lambda: e.genotype_catalog(texts, K, Q), lambda: e.genotype_partial_catalog(texts, K, Q))
        prepared_calls = (lambda: e.genotype_prepared(cat), lambda: e.genotype_partial_prepared(cat))
        for what, calls in (("the text-taking calls", text_calls), ("the prepared calls", prepared_calls)):
            for first in (0, 1):                                            # the genotype first, then the partial genotype first
                got = {k: calls[k]() for k in (first, 1 - first)}
                assert _same(got[0], sg) and _same(got[1], spg), (what, first)
                _both_kept(e, alone)
        # a failed call forgets its own kind's rows and leaves the other's
        with pytest.raises(mtr_amd.MtrError, match="gain = 0"):
            e.genotype_catalog(texts, K, Q, gain=0)
        assert not _kept(e, False) and _kept(e, True)
        assert _same(e._partial_catalog_rows(len(texts), spg.read.numel(), spg.candidates), spg) and e.test_partial_catalog_stats()[0] == alone[1][1]
        with pytest.raises(mtr_amd.MtrError, match="no catalogue call"):
            e.test_catalog_stats()
        assert _same(e.genotype_prepared(cat), sg)
        with pytest.raises(mtr_amd.MtrError, match="max_tail = -1"):
            e.genotype_partial_prepared(cat, max_tail=-1)
        assert _kept(e, False) and not _kept(e, True)
        assert _same(e._catalog_rows(len(texts), sg.read.numel(), sg.candidates), sg) and e.test_catalog_stats()[0] == alone[0][1]
        # an upload forgets both
        assert _same(e.genotype_partial_prepared(cat), spg)
        _both_kept(e, alone)
        e.upload(reads[:2])
        assert not _kept(e, False) and not _kept(e, True)
        cat.close()
    finally:
        e.close()
