"""Allele calls on the MI355X (mtr_call_alleles_device, Engine.call_alleles, the kernels of mtr_amd/csrc/allele_call.hip.inc).

Truth is tests/allele_call_ref.py, the definition of include/mtr_hip.h in numpy; tests/test_allele_call_ref.py holds it to hand-worked lists and
shows that the inputs of tests/allele_call_cases.py are not degenerate.  Everything is exact equality: every column, every dtype, every shape.
The inputs are Genotypes columns built in numpy and moved to the device - no reads and no DP - except in the last test, which goes from reads
through genotype_loci."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import allele_call_cases as cases
from tests import allele_call_ref as aref
from tests import flank_ref as fref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _device(rows, eng):
    """the four columns the call reads on the device, the three others absent"""
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return mtr_amd.Genotypes(t(rows.spanning), None, None, t(rows.window), t(rows.fields), None, t(rows.ratio))


def _assert_calls(got, want, what=""):
    for name, g, w in zip(mtr_amd.AlleleCalls._fields, (t.cpu().numpy() for t in got), want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError((what, name, at.tolist(), g[tuple(at)].tolist(), w[tuple(at)].tolist()))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _sweep(eng, rows, what):
    gt = _device(rows, eng)
    for measure in ("copies", "bases"):
        for rule in cases.SWEEP:
            want, _ = aref.call_alleles(rows, mtr_amd.ALLELE_BASES if measure == "bases" else mtr_amd.ALLELE_COPIES, cases.MIN_RATIO, *rule)
            got = eng.call_alleles(gt, measure, cases.MIN_RATIO, *rule)
            _assert_calls(got, want, f"{what}, {measure}, {rule}")
            assert _same(got, eng.call_alleles(gt, measure, cases.MIN_RATIO, *rule)), (what, measure, rule)


def test_tile_edges(eng):
    """3000 reads x 16 loci whose support counts sit below, at and above the wavefront, the tile and its multiples; the last locus' cost1 is over
    2^31 under bases"""
    rows = cases.tile_edges()
    _sweep(eng, rows, "tile edges")
    got = eng.call_alleles(_device(rows, eng), "bases", cases.MIN_RATIO, 3, 20, 2)
    assert int(got.cost[-1, 0]) > 2 ** 31 and np.diff(got.support_off.cpu().numpy()).tolist() == list(cases.EDGE_SUPPORT)


@pytest.mark.parametrize("swap", [False, True], ids=["as_built", "loci_reversed"])
def test_many_loci(eng, swap):
    rows = cases.many_loci(swap)
    assert rows.spanning.shape == (40, 700)
    _sweep(eng, rows, f"many loci, swap {swap}")


@pytest.mark.parametrize("m", [63, 64, 65])
def test_either_side_of_the_loci_count_from_which_every_lane_counts_for_itself(eng, m):
    _sweep(eng, cases.lane_edges(m), f"{m} loci")


@pytest.mark.parametrize("m", [cases.SPREAD_LOCI, cases.SPREAD_LOCI + 1])
def test_either_side_of_the_loci_count_up_to_which_the_counters_are_spread(eng, m):
    rows = cases.spread_edges(m)
    gt = _device(rows, eng)
    for measure, rule in ((mtr_amd.ALLELE_COPIES, cases.SWEEP[0]), (mtr_amd.ALLELE_BASES, cases.SWEEP[1])):
        want, _ = aref.call_alleles(rows, measure, cases.MIN_RATIO, *rule)
        _assert_calls(eng.call_alleles(gt, measure, cases.MIN_RATIO, *rule), want, f"{m} loci, {measure}, {rule}")
    assert set(want[4].tolist()) == {0, 1, 2}


def test_the_hand_worked_lists_and_the_empty_windows(eng):
    _sweep(eng, cases.from_lists(), "hand")
    got = eng.call_alleles(_device(cases.from_lists(), eng), "copies", cases.MIN_RATIO, 3, 20, 2)
    assert got.zygosity.cpu().tolist()[:3] == [2, 1, 2] and got.call.cpu().tolist()[:3] == [[20, 35], [10, 10], [10, 40]]
    assert got.call_support.cpu().tolist()[2] == [3, 6] and got.cost.cpu().tolist()[:3] == [[76, 4], [30, 30], [180, 90]]
    rows = cases.empty_windows()
    want, _ = aref.call_alleles(rows, 0, 1.0, 2, 20, 1)
    got = eng.call_alleles(_device(rows, eng), mtr_amd.ALLELE_COPIES, 1.0, 2, 20, 1)
    _assert_calls(got, want, "min_ratio = 1")
    assert got.value.cpu().tolist() == [0, 0, 0, 6] and got.read.cpu().tolist() == [0, 2, 3, 1]


def test_smallest(eng):
    for supported in (True, False):
        rows = cases.smallest(supported)
        want, _ = aref.call_alleles(rows, 0, cases.MIN_RATIO, 1, 0, 1)
        got = eng.call_alleles(_device(rows, eng), "copies", cases.MIN_RATIO, 1, 0, 1)        # (S == 0: the S-sized destination pointers are NULL)
        _assert_calls(got, want, f"one row, supported {supported}")
        assert got.value.numel() == int(supported) and got.zygosity.cpu().tolist() == [int(supported)] and got.support_off.cpu().tolist() == [0, int(supported)]


# ---- protocol ---------------------------------------------------------------------------------------------------------------------------
def _dst(dev, m, S):
    shapes = ((m + 1, torch.int64), (S, torch.int32), (S, torch.int32), (S, torch.uint8), (m, torch.uint8), (2 * m, torch.int32), (2 * m, torch.int32), (2 * m, torch.int64))
    return [torch.full((max(n, 1),), 77, dtype=t, device=dev) for n, t in shapes]


def test_the_argument_errors_the_capacities_and_the_destination_stays(eng):
    rows = cases.from_lists()
    n, m = rows.spanning.shape
    gt = _device(rows, eng)
    dev = torch.device("cuda", eng.device)
    want, _ = aref.call_alleles(rows, 0, cases.MIN_RATIO, 3, 20, 2)
    S = int(want[0][-1])
    cols = _dst(dev, m, S)
    ptrs = [c.data_ptr() for c in cols]
    host = np.zeros(n * m * 8, np.int32)
    far = torch.zeros(16, dtype=torch.uint8, device=dev)
    # (tensors of this size are allocations of their own, and the 16 bytes lie in a block of a few MB)
    R = 2 ** 24
    large = [torch.empty(R, dtype=torch.uint8, device=dev), torch.empty(2 * R, dtype=torch.int32, device=dev), torch.empty(8 * R, dtype=torch.int32, device=dev)]
    big = dict(n_reads=R, n_loci=1, cap_rows=R, spanning=large[0].data_ptr(), window=large[1].data_ptr(), fields=large[2].data_ptr())
    torch.cuda.synchronize()
    full = dict(spanning=gt.spanning.data_ptr(), window=gt.window.data_ptr(), fields=gt.fields.data_ptr(), ratio=gt.ratio.data_ptr(), cap_rows=n * m)

    def call(n_reads=n, n_loci=m, prm=(0, cases.MIN_RATIO, 3, 20, 2), dst=None, rows_null=False, prm_null=False, out_null=False, **over):
        r = mtr_amd.CGenotypesDst(**{**full, **over})
        p = mtr_amd.CAlleleParams(*prm)
        ns = C.c_int64(-7)
        st = eng.lib.mtr_call_alleles_device(eng.h, None if rows_null else C.byref(r), n_reads, n_loci, None if prm_null else C.byref(p), None,
                                             None if dst is None else C.byref(dst), None if out_null else C.byref(ns))
        return mtr_amd.STATUS.get(st, st), int(ns.value), eng.lib.mtr_last_error(eng.h).decode()

    whole = mtr_amd.CAlleleCallsDst(*ptrs, m, S)
    assert call(dst=whole, out_null=True)[0] == "MTR_ERR_BAD_ARG"
    for kw, word in ((dict(rows_null=True), "rows"), (dict(prm_null=True), "prm"), (dict(n_reads=0), "n_reads"), (dict(n_loci=0), "n_loci"),
                     (dict(n_reads=2 ** 31, n_loci=1, cap_rows=2 ** 31), "2^31 - 1"), (dict(n_reads=2 ** 27, n_loci=16, cap_rows=2 ** 31), "2^31 - 1"),
                     (dict(prm=(2, 0.5, 3, 20, 2)), "measure"), (dict(prm=(-1, 0.5, 3, 20, 2)), "measure"), (dict(prm=(0, -0.1, 3, 20, 2)), "min_ratio"),
                     (dict(prm=(0, 1.5, 3, 20, 2)), "min_ratio"), (dict(prm=(0, float("nan"), 3, 20, 2)), "min_ratio"), (dict(prm=(0, 0.5, 0, 20, 2)), "min_support"),
                     (dict(prm=(0, 0.5, 3, -1, 2)), "min_percent"), (dict(prm=(0, 0.5, 3, 51, 2)), "min_percent"), (dict(prm=(0, 0.5, 3, 20, 0)), "min_sep"),
                     (dict(prm=(7, 9.0, 0, 99, 0)), "measure"), (dict(prm=(0, 9.0, 0, 99, 0)), "min_ratio"),        # the first offender in the table's order
                     (dict(prm=(0, 0.5, 0, 99, 0)), "min_support"), (dict(prm=(0, 0.5, 1, 99, 0)), "min_percent"), (dict(n_loci=0, prm=(7, 0.5, 3, 20, 2)), "n_loci"),
                     (dict(spanning=None), "column"), (dict(window=None), "column"), (dict(fields=None), "column"), (dict(ratio=None), "column"),
                     (dict(cap_rows=n * m - 1), "cap_rows"), (dict(ratio=None, prm=(0, 0.5, 3, 20, 0)), "min_sep"),
                     (dict(fields=host.ctypes.data), "fields is not device memory"), (dict(ratio=host.ctypes.data), "ratio is not device memory"),
                     # past the end of an allocation, column by column: 2^24 rows against a tensor of 16 bytes, the columns before it large enough
                     (dict(big, spanning=far.data_ptr()), "spanning's allocation"), (dict(big, window=far.data_ptr()), "window's allocation"),
                     (dict(big, fields=far.data_ptr()), "fields's allocation"), (dict(big, ratio=far.data_ptr()), "ratio's allocation")):
        st, got_S, msg = call(dst=whole, **kw)
        assert st == "MTR_ERR_BAD_ARG" and word in msg and got_S == 0, (kw, st, msg, got_S)
    # the three unread columns may be anything
    assert call(orientation=1, flank_dist=2, score=3)[:2] == ("MTR_OK", S)
    # the size alone; each capacity; a NULL column of each kind
    assert call()[:2] == ("MTR_OK", S) and S == sum(len(v) for v in cases.HAND)
    st, got_S, msg = call(dst=mtr_amd.CAlleleCallsDst(*ptrs, m - 1, S))
    assert (st, got_S) == ("MTR_ERR_OVERFLOW", S) and "loci" in msg
    st, got_S, msg = call(dst=mtr_amd.CAlleleCallsDst(*ptrs, m, S - 1))
    assert (st, got_S) == ("MTR_ERR_OVERFLOW", S) and "supporting" in msg
    for k in range(8):
        st, got_S, msg = call(dst=mtr_amd.CAlleleCallsDst(*ptrs[:k], None, *ptrs[k + 1:], m, S))
        assert (st, got_S) == ("MTR_ERR_BAD_ARG", S) and "destination column" in msg, (k, st, msg)
    # a negative value in a supporting row: with min_ratio = 0 the dropped rows support, and some of them hold negative copies
    ok0, _ = (rows.spanning == 1), None
    neg = np.argwhere(ok0 & (rows.fields[:, :, 3] < 0))
    assert len(neg) >= 2
    first = int(neg[0][0]) * m + int(neg[0][1])
    st, _, msg = call(dst=whole, prm=(0, 0.0, 3, 20, 2))
    assert st == "MTR_ERR_BAD_ARG" and f"row {first} " in msg and f"read {first // m}, locus {first % m}" in msg, msg
    assert call(prm=(0, 0.0, 3, 20, 2))[0] == "MTR_ERR_BAD_ARG"
    torch.cuda.synchronize()
    assert all(bool((c == 77).all()) for c in cols)
    # then the same destination filled by a correct call
    assert call(dst=whole)[:2] == ("MTR_OK", S)
    torch.cuda.synchronize()
    got = [c[:k] for c, k in zip(cols, (m + 1, S, S, S, m, 2 * m, 2 * m, 2 * m))]
    got = mtr_amd.AlleleCalls(*got[:5], got[5].reshape(m, 2), got[6].reshape(m, 2), got[7].reshape(m, 2))
    _assert_calls(got, want, "after the errors")
    # the Python edge
    with pytest.raises(mtr_amd.MtrError, match="measure"):
        eng.call_alleles(gt, "length")
    with pytest.raises(mtr_amd.MtrError, match="measure"):
        eng.call_alleles(gt, 2)
    with pytest.raises(mtr_amd.MtrError, match="min_percent"):
        eng.call_alleles(gt, "copies", cases.MIN_RATIO, 3, 60, 2)
    with pytest.raises(mtr_amd.MtrError, match="must be GPU tensors"):
        eng.call_alleles(mtr_amd.Genotypes(*[None if c is None else c.cpu() for c in gt]))
    _assert_calls(eng.call_alleles(gt, 0, cases.MIN_RATIO, 3, 20, 2), want, "the measure as an integer")


def test_a_fresh_engine_with_nothing_uploaded():
    e = mtr_amd.Engine()
    try:
        rows = cases.from_lists()
        want, _ = aref.call_alleles(rows, 1, cases.MIN_RATIO, 2, 20, 1)
        _assert_calls(e.call_alleles(_device(rows, e), "bases", cases.MIN_RATIO), want, "no batch")
    finally:
        e.close()


def _texts(loci):
    return [tuple(fref.text(s) for s in locus) for locus in loci]


def test_a_call_leaves_the_run_the_report_and_the_genotype_alone(eng):
    reads, loci = cases.e2e()
    eng.upload(reads)
    eng.run()
    rec, rep, gt = eng.fetch(), eng.report_tensors(), eng.genotype_loci(_texts(loci), cases.E2E_K)
    calls = eng.call_alleles(gt, "copies", cases.E2E_MIN_RATIO, *cases.E2E_RULE)
    assert int(calls.support_off[-1]) == 22
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    assert _same(eng.report_tensors(), rep) and _same(eng.genotype_loci(_texts(loci), cases.E2E_K), gt)
    assert _same(eng.call_alleles(gt, "copies", cases.E2E_MIN_RATIO, *cases.E2E_RULE), calls)


def test_end_to_end_and_batches(eng):
    """reads -> genotype_loci -> call_alleles: the reference on the GPU's own genotype columns, the alleles the reads were built with, and two
    batches joined with torch.cat equal to the one batch column for column"""
    reads, loci = cases.e2e()
    eng.upload(reads)
    gt = eng.genotype_loci(_texts(loci), cases.E2E_K)
    host = cases.Rows(*[c.cpu().numpy() for c in (gt.spanning, gt.window, gt.fields, gt.ratio)])
    results = {}
    for measure, sep, alleles in ((mtr_amd.ALLELE_COPIES, 2, [[5, 12], [8, 8]]), (mtr_amd.ALLELE_BASES, 6, [[15, 36], [48, 48]])):
        rule = cases.E2E_RULE[:2] + (sep,)
        want, _ = aref.call_alleles(host, measure, cases.E2E_MIN_RATIO, *rule)
        got = eng.call_alleles(gt, measure, cases.E2E_MIN_RATIO, *rule)
        _assert_calls(got, want, f"end to end, measure {measure}")
        assert got.zygosity.cpu().tolist() == [2, 1] and got.call.cpu().tolist() == alleles and got.call_support.cpu().tolist() == [[9, 7], [6, 0]]
        results[measure] = got
    text = mtr_amd.format_allele_calls(_texts(loci), results[mtr_amd.ALLELE_COPIES])
    assert text.count(b"\n") == 2 and text.startswith(b"0\t16\t2\t5\t12\t9\t7\t")
    # the same reads as two batches, each genotyped, the rows joined along the read axis
    parts = []
    for batch in (reads[:11], reads[11:]):
        eng.upload(batch)
        parts.append(eng.genotype_loci(_texts(loci), cases.E2E_K))
    joined = mtr_amd.Genotypes(*[torch.cat(cols, dim=0) for cols in zip(*parts)])
    assert _same(joined, gt)
    for measure, sep in ((mtr_amd.ALLELE_COPIES, 2), (mtr_amd.ALLELE_BASES, 6)):
        assert _same(eng.call_alleles(joined, measure, cases.E2E_MIN_RATIO, *cases.E2E_RULE[:2], sep), results[measure]), measure
