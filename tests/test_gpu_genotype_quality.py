"""Genotype quality on the MI355X (mtr_genotype_quality_device, Engine.genotype_quality, the kernels of mtr_amd/csrc/genotype_quality.hip.inc).

Truth is tests/genotype_quality_ref.py, the definition of include/mtr_hip.h in plain Python; tests/test_genotype_quality_ref.py holds it to an
unbanded alignment and shows that the inputs of tests/genotype_quality_cases.py meet the situations they are there for.  Everything is exact
equality: every column, every dtype, every shape - with the qualities and without, with several alignments per wavefront (the default) and with
MTR_TEST_GQ_ROWS=0, one per wavefront."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import mtr_amd
from tests import consensus_cases as cc
from tests import consensus_quality_cases as cqc
from tests import genotype_quality_cases as gc
from tests import genotype_quality_ref as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", eng.device))


def _inputs(eng, d, with_qual=True):
    case = d["case"]
    sg = SimpleNamespace(n_loci=case["n_loci"], read=_dev(eng, case["read"]), locus=_dev(eng, case["locus"]))
    win = mtr_amd.GenotypeWindows(_dev(eng, case["win_off"]), _dev(eng, case["win_bases"]))
    calls = SimpleNamespace(support_off=_dev(eng, case["support_off"]), read=_dev(eng, case["sup_read"]), allele=_dev(eng, case["allele"]), zygosity=_dev(eng, case["zygosity"]))
    cons = SimpleNamespace(off=_dev(eng, d["cons_off"]), bases=_dev(eng, d["cons_bases"]))
    return sg, win, _dev(eng, d["qual"]) if with_qual else None, calls, cons


def _assert_columns(got, want, what=""):
    for name, g, w in zip(ref.COLUMNS, (t.cpu().numpy() for t in got), want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError((what, name, at.tolist(), g[tuple(at)].tolist(), w[tuple(at)].tolist()))


def _call(eng, d, with_qual=True, prm=None):
    prm = prm or d["prm"]
    return eng.genotype_quality(*_inputs(eng, d, with_qual), band_extra=prm[0], qual_cap=prm[1], gap_cap=prm[2], read_cap=prm[3])


@pytest.mark.parametrize("rows", ["several", "one"])
@pytest.mark.parametrize("name", sorted(gc.all_cases()))
def test_every_column_equals_the_reference(eng, monkeypatch, name, rows):
    if rows == "one":
        monkeypatch.setenv("MTR_TEST_GQ_ROWS", "0")
    else:
        monkeypatch.delenv("MTR_TEST_GQ_ROWS", raising=False)
    d, want, want_none = gc.expected()[name]
    got = _call(eng, d)
    _assert_columns(got, want, (name, rows, "qual"))
    _assert_columns(_call(eng, d, with_qual=False), want_none, (name, rows, "None"))
    again = _call(eng, d)
    assert all(torch.equal(x, y) for x, y in zip(got, again)), name


# ---- the properties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["truth1", "members", "lengths"])
def test_unit_weights_are_the_consensus_distance_and_a_constant_quality_its_multiple(eng, name):
    """against eng.allele_consensus' own inputs and result: consensus_cases' columns, the sequences the GPU voted"""
    from tests import consensus_ref as cref

    case = cc.all_cases()[name]
    extra = case["band_extra"]
    d = dict(case=case, qual=np.random.default_rng(3).integers(0, 94, size=len(case["win_bases"])).astype(np.uint8), cons_off=None, cons_bases=None, prm=(extra, 1, 1, 60))
    sg, win, qual, calls, _ = _inputs(eng, dict(d, cons_off=np.zeros(1, np.int64), cons_bases=np.zeros(0, np.uint8)))
    cons = eng.allele_consensus(sg, win, calls, band_extra=extra)
    off, bases = cons.off.cpu().numpy(), cons.bases.cpu().numpy()
    unit = eng.genotype_quality(sg, win, qual, calls, cons, band_extra=extra, qual_cap=1, gap_cap=1, read_cap=60).score.cpu().numpy()
    # the unit-cost distance by the consensus' reference matrix, entry by entry
    row_of = {(int(r), int(l)): k for k, (r, l) in enumerate(zip(case["read"], case["locus"]))}
    checked = 0
    for l in range(case["n_loci"]):
        z = int(case["zygosity"][l])
        seqs = [bases[off[2 * l + a]:off[2 * l + a + 1]].tolist() for a in range(z)]
        for e in range(int(case["support_off"][l]), int(case["support_off"][l + 1])):
            r = row_of[(int(case["sup_read"][e]), l)]
            W = case["win_bases"][case["win_off"][r]:case["win_off"][r + 1]].tolist()
            if z == 0 or any(cref.skipped(len(W), len(Cs), extra) for Cs in seqs):
                assert unit[e].tolist() == [-1, -1]
                continue
            for a, Cs in enumerate(seqs):
                assert unit[e, a] == cref.matrix(W, Cs, extra)[0][len(W)][len(Cs)], (name, e, a)
                checked += 1
    assert checked > 0
    if (case["win_off"][1:] > case["win_off"][:-1]).all():          # no empty window: one constant quality c <= gap_cap multiplies every score
        flat = torch.full_like(qual, 7)
        seven = eng.genotype_quality(sg, win, flat, calls, cons, band_extra=extra, qual_cap=40, gap_cap=9, read_cap=60).score.cpu().numpy()
        assert np.array_equal(seven, np.where(unit < 0, -1, 7 * unit))


# ---- the protocol -------------------------------------------------------------------------------------------------------------------------------
def _dst_columns(eng, m, S):
    dev = torch.device("cuda", eng.device)
    shapes = (((S, 2), torch.int32), ((S,), torch.uint8), ((S,), torch.int32), ((m, 3), torch.int64), ((m, 3), torch.int64), ((m,), torch.uint8), ((m,), torch.int64),
              ((m,), torch.int32), ((m,), torch.int32))
    return [torch.full(shape, 77, dtype=t, device=dev) for shape, t in shapes]


def test_the_refusals_write_nothing_and_the_next_call_succeeds(eng):
    d, want, _ = gc.expected()["zygosity"]
    case = d["case"]
    sg, win, qual, calls, cons = _inputs(eng, d)
    prm = d["prm"]
    args = dict(band_extra=prm[0], qual_cap=prm[1], gap_cap=prm[2], read_cap=prm[3])
    for name, bad in (("band_extra", -1), ("band_extra", 65), ("qual_cap", 0), ("qual_cap", 94), ("gap_cap", 0), ("gap_cap", 41), ("read_cap", 0), ("read_cap", (1 << 20) + 1)):
        with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: {name}"):
            eng.genotype_quality(sg, win, qual, calls, cons, **dict(args, **{name: bad}))
    for first, second in (("band_extra", "qual_cap"), ("qual_cap", "gap_cap"), ("gap_cap", "read_cap")):          # the parameters in struct order
        with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: {first}"):
            eng.genotype_quality(sg, win, qual, calls, cons, **dict(args, **{first: 1000, second: 0}))
    swapped, locus_swapped = case["read"].copy(), case["locus"].copy()
    swapped[[4, 5]], locus_swapped[[4, 5]] = swapped[[5, 4]], locus_swapped[[5, 4]]
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: row 5 is out of order"):
        eng.genotype_quality(SimpleNamespace(n_loci=sg.n_loci, read=_dev(eng, swapped), locus=_dev(eng, locus_swapped)), win, qual, calls, cons, **args)
    lost = case["sup_read"].copy()
    lost[7] = int(case["read"].max()) + 1
    with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: support entry 7 \(read \d+\) has no row"):
        eng.genotype_quality(sg, win, qual, SimpleNamespace(support_off=calls.support_off, read=_dev(eng, lost), allele=calls.allele, zygosity=calls.zygosity), cons, **args)
    off = d["cons_off"].copy()
    off[4] = off[5] + 1
    with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: allele 4 \(locus 2\): cons_off does not ascend"):
        eng.genotype_quality(sg, win, qual, calls, SimpleNamespace(off=_dev(eng, off), bases=cons.bases), **args)
    # short capacities and each NULL column, through the C entry: nothing is written; then the call succeeds
    m, S = case["n_loci"], len(case["sup_read"])
    src = mtr_amd.CConsensusSrc(sg.read.data_ptr(), sg.locus.data_ptr(), win.off.data_ptr(), win.bases.data_ptr(), calls.support_off.data_ptr(), calls.read.data_ptr(),
                                calls.allele.data_ptr(), calls.zygosity.data_ptr(), sg.read.numel(), win.bases.numel(), S, m)
    params = mtr_amd.CGqParams(*prm)
    cols = _dst_columns(eng, m, S)
    ptrs = [c.data_ptr() for c in cols]
    torch.cuda.synchronize()
    raw = lambda *a: mtr_amd.STATUS[eng.lib.mtr_genotype_quality_device(eng.h, C.byref(src), qual.data_ptr(), cons.off.data_ptr(), cons.bases.data_ptr(), cons.bases.numel(),      # noqa: E731
                                                                        C.byref(params), None, C.byref(mtr_amd.CGqDst(*a)))]
    assert raw(*ptrs, S - 1, m) == "MTR_ERR_OVERFLOW" and raw(*ptrs, S, m - 1) == "MTR_ERR_OVERFLOW"
    for k in range(9):
        assert raw(*ptrs[:k], None, *ptrs[k + 1:], S, m) == "MTR_ERR_BAD_ARG", ref.COLUMNS[k]
        assert "a destination column is NULL" in eng.lib.mtr_last_error(eng.h).decode()
    assert mtr_amd.STATUS[eng.lib.mtr_genotype_quality_device(eng.h, C.byref(src), qual.data_ptr(), cons.off.data_ptr(), cons.bases.data_ptr(), cons.bases.numel(), C.byref(params), None,
                                                              None)] == "MTR_ERR_BAD_ARG"
    assert mtr_amd.STATUS[eng.lib.mtr_genotype_quality_device(eng.h, C.byref(src), qual.data_ptr(), None, cons.bases.data_ptr(), cons.bases.numel(), C.byref(params), None,
                                                              C.byref(mtr_amd.CGqDst(*ptrs, S, m)))] == "MTR_ERR_BAD_ARG"
    assert "an input column is NULL" in eng.lib.mtr_last_error(eng.h).decode()
    assert all((c == 77).all() for c in cols)
    assert raw(*ptrs, S, m) == "MTR_OK"
    _assert_columns(cols, want, "after the refusals")


# ---- from FASTQ bytes to a genotype quality -------------------------------------------------------------------------------------------------------
def test_from_fastq_bytes_to_a_confident_heterozygous_call_and_back(eng):
    seed = gc.GQ_SEED
    reads, loci, truth = cqc.fq_reads(seed), cc.truth_loci(), cc.truth_alleles()
    n = 2 * cqc.FQ_READS
    buf = _dev(eng, np.frombuffer(cqc.fastq_bytes(reads), np.uint8).copy())
    eng.upload_fastq_device(buf, keep_quality=True)
    sg = eng.genotype_catalog(loci, 1)
    win, qual = eng.genotype_windows(sg), eng.genotype_window_qualities(sg)
    assert sg.read.cpu().tolist() == list(range(n)) and sg.locus.cpu().tolist() == [0] * n
    calls = eng.call_alleles(sg, "bases")
    assert calls.zygosity.cpu().tolist() == [2, 0]
    cons = eng.allele_consensus(sg, win, calls, band_extra=cqc.FQ_EXTRA)
    off = cons.off.cpu().tolist()
    assert [cons.bases[off[a]:off[a + 1]].cpu().tolist() for a in (0, 1)] == [t.tolist() for t in truth]
    gq = eng.genotype_quality(sg, win, qual, calls, cons, band_extra=cqc.FQ_EXTRA)
    case, q = cqc.fq_case(seed)                                                        # the same windows, qualities and list order as columns: the reference's answer
    assert np.array_equal(qual.cpu().numpy(), q) and calls.read.cpu().tolist() == case["sup_read"].tolist()
    _assert_columns(gq, ref.genotype_quality(case, q, cons.off.cpu().numpy(), cons.bases.cpu().numpy(), (cqc.FQ_EXTRA, 40, 20, 60)), "fastq")
    assert gq.gt.cpu().tolist() == [1, 255] and int(gq.gq[0]) > 0
    assert gq.best.cpu().tolist() == [r // cqc.FQ_READS for r in calls.read.cpu().tolist()]                  # read a * FQ_READS + k is allele a's
    text = mtr_amd.format_genotype_quality(loci, calls, gq).decode().splitlines()
    assert text[0].split("\t")[-4:-2] == ["0/1", str(int(gq.gq[0]))] and text[0].split("\t")[-1] == f"{n}/0" and text[1].split("\t")[-4:] == ["./.", "-1", "-1,-1,-1", "0/0"]
    for side in (0, 1):                                                                # one allele's reads alone, the calls forced to zygosity 2 over them
        one = gc.one_side(case, side)
        forced = mtr_amd.AlleleCalls(_dev(eng, one["support_off"]), _dev(eng, np.zeros(len(one["sup_read"]), np.int32)), _dev(eng, one["sup_read"]), _dev(eng, one["allele"]),
                                     calls.zygosity, calls.call, calls.call_support, calls.cost)
        hom = eng.genotype_quality(sg, win, qual, forced, cons, band_extra=cqc.FQ_EXTRA)
        assert hom.gt.cpu().tolist() == [2 * side, 255] and int(hom.gq[0]) > 0, side
    # a second round.  Where every read is on its side nothing moves ...
    again = mtr_amd.with_reassigned_alleles(calls, gq)
    assert all(torch.equal(x, y) for x, y in zip(again, calls))
    # ... so two reads are put on the wrong side by hand (gc.mixed_order: the entries either side of the alleles' border swap alleles).  The consensus over
    # those calls misses the truth; the scores against the true sequences send both reads back, and the second round votes the two true alleles
    order, wrong = gc.mixed_order(case)
    at = _dev(eng, order)
    mixed = mtr_amd.AlleleCalls(calls.support_off, calls.value[at], calls.read[at], _dev(eng, wrong), calls.zygosity, calls.call, calls.call_support, calls.cost)
    seqs = lambda c: [c.bases[o:p].cpu().tolist() for o, p in zip(c.off.cpu().tolist()[:2], c.off.cpu().tolist()[1:3])]      # noqa: E731
    assert seqs(eng.allele_consensus(sg, win, mixed, band_extra=cqc.FQ_EXTRA)) != [t.tolist() for t in truth]
    mixed_gq = eng.genotype_quality(sg, win, qual, mixed, cons, band_extra=cqc.FQ_EXTRA)
    assert mixed_gq.best.cpu().tolist() != wrong.tolist() and mixed_gq.best.cpu().tolist() == [r // cqc.FQ_READS for r in mixed.read.cpu().tolist()]
    fixed = mtr_amd.with_reassigned_alleles(mixed, mixed_gq)
    assert not torch.equal(fixed.read, mixed.read) and fixed.allele.cpu().tolist() == [0] * cqc.FQ_READS + [1] * cqc.FQ_READS
    assert [r // cqc.FQ_READS for r in fixed.read.cpu().tolist()] == fixed.allele.cpu().tolist() and fixed.call_support.cpu().tolist() == [[cqc.FQ_READS] * 2, [0, 0]]
    assert seqs(eng.allele_consensus(sg, win, fixed, band_extra=cqc.FQ_EXTRA)) == [t.tolist() for t in truth]
