"""Allele calls by sequence on the MI355X (mtr_call_alleles_sequence_device, mtr_call_alleles_sequence_copy_device,
Engine.call_alleles_by_sequence, the kernels of mtr_amd/csrc/seq_calls.hip.inc).

Truth is tests/seq_calls_ref.py, the definition of include/mtr_hip.h in plain Python; tests/test_seq_calls_ref.py holds it to brute force and shows
that the inputs of tests/seq_calls_cases.py meet the situations they are there for.  Everything is exact equality: every column, every dtype,
every shape - with four alignments per wavefront (the default) and with MTR_TEST_SEQ_ROWS=0, one per wavefront."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import mtr_amd
from tests import consensus_cases as cc
from tests import seq_calls_cases as sc
from tests import seq_calls_ref as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", eng.device))


def _inputs(eng, case):
    sg = SimpleNamespace(n_loci=case["n_loci"], read=_dev(eng, case["read"]), locus=_dev(eng, case["locus"]))
    win = mtr_amd.GenotypeWindows(_dev(eng, case["win_off"]), _dev(eng, case["win_bases"]))
    calls = SimpleNamespace(support_off=_dev(eng, case["support_off"]), read=_dev(eng, case["sup_read"]), value=_dev(eng, case["value"]))
    return sg, win, calls


def _columns(got):
    """a SequenceCalls in the reference's column order"""
    return (*got.calls, *got[1:])


def _assert_calls(got, want, what=""):
    for name, g, w in zip(ref.COLUMNS, (t.cpu().numpy() for t in got), want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError((what, name, at.tolist(), g[tuple(at)].tolist(), w[tuple(at)].tolist()))


def _call(eng, case, prm):
    return eng.call_alleles_by_sequence(*_inputs(eng, case), max_dist=prm[0], min_support=prm[1], min_percent=prm[2], min_sep=prm[3], min_gain=prm[4])


@pytest.mark.parametrize("rows", ["four", "one"])
@pytest.mark.parametrize("name", sorted(sc.all_cases()))
def test_every_column_equals_the_reference(eng, monkeypatch, name, rows):
    if rows == "one":
        monkeypatch.setenv("MTR_TEST_SEQ_ROWS", "0")
    else:
        monkeypatch.delenv("MTR_TEST_SEQ_ROWS", raising=False)
    case, prm, want = sc.expected()[name]
    got = _call(eng, case, prm)
    _assert_calls(_columns(got), want, (name, rows))
    again = _call(eng, case, prm)
    assert all(torch.equal(x, y) for x, y in zip(_columns(got), _columns(again))), name


# ---- the protocol -------------------------------------------------------------------------------------------------------------------------------
def _raw(eng, case, prm, value=True):
    sg, win, calls = _inputs(eng, case)
    src = mtr_amd.CConsensusSrc(sg.read.data_ptr(), sg.locus.data_ptr(), win.off.data_ptr(), win.bases.data_ptr(), calls.support_off.data_ptr(), calls.read.data_ptr(), None, None,
                                sg.read.numel(), win.bases.numel(), calls.read.numel(), case["n_loci"])
    ns, npairs = C.c_int64(-1), C.c_int64(-1)
    params = mtr_amd.CSeqParams(*prm)
    st = eng.lib.mtr_call_alleles_sequence_device(eng.h, C.byref(src), calls.value.data_ptr() if value else None, C.byref(params), None, C.byref(ns), C.byref(npairs))
    return mtr_amd.STATUS[st], ns.value, npairs.value, (sg, win, calls)


def _dst_columns(eng, m, S, P):
    dev = torch.device("cuda", eng.device)
    shapes = (((m + 1,), torch.int64), ((S,), torch.int32), ((S,), torch.int32), ((S,), torch.uint8), ((m,), torch.uint8), ((m, 2), torch.int32), ((m, 2), torch.int32),
              ((m, 2), torch.int64), ((m, 2), torch.int32), ((S,), torch.int32), ((m,), torch.uint8), ((m + 1,), torch.int64), ((P,), torch.uint8))
    return [torch.full(shape, 77, dtype=t, device=dev) for shape, t in shapes]


def test_copy_without_compute_fails_and_a_refused_call_keeps_nothing():
    fresh = mtr_amd.Engine()
    case, prm, want = sc.expected()["ties"]
    m, S, P = case["n_loci"], len(case["sup_read"]), len(want[-1])
    cols = _dst_columns(fresh, m, S, P)
    dst = mtr_amd.CSeqCallsDst(*[c.data_ptr() for c in cols], m, S, P)
    torch.cuda.synchronize()
    assert mtr_amd.STATUS[fresh.lib.mtr_call_alleles_sequence_copy_device(fresh.h, C.byref(dst))] == "MTR_ERR_BAD_ARG"
    assert _raw(fresh, case, prm)[:3] == ("MTR_OK", S, P)
    assert _raw(fresh, case, (255,) + prm[1:])[:3] == ("MTR_ERR_BAD_ARG", 0, 0)          # a refused call: what the one before kept is gone
    assert mtr_amd.STATUS[fresh.lib.mtr_call_alleles_sequence_copy_device(fresh.h, C.byref(dst))] == "MTR_ERR_BAD_ARG"
    assert all((c == 77).all() for c in cols)
    assert _raw(fresh, case, prm)[:3] == ("MTR_OK", S, P)
    assert fresh.lib.mtr_call_alleles_sequence_copy_device(fresh.h, C.byref(dst)) == 0
    _assert_calls(cols, want, "after the refusals")
    fresh.close()


def test_the_refusals_write_nothing_and_the_next_call_succeeds(eng):
    case, prm, want = sc.expected()["many"]
    sg, win, calls = _inputs(eng, case)
    args = dict(max_dist=prm[0], min_support=prm[1], min_percent=prm[2], min_sep=prm[3], min_gain=prm[4])
    for name, bad, word in (("max_dist", -1, "max_dist"), ("max_dist", 255, "max_dist"), ("min_support", 0, "min_support"), ("min_percent", 51, "min_percent"), ("min_sep", 0, "min_sep"),
                            ("min_gain", 101, "min_gain"), ("min_gain", -1, "min_gain")):
        with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: {word}"):
            eng.call_alleles_by_sequence(sg, win, calls, **dict(args, **{name: bad}))
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: max_dist"):                # the parameters in struct order
        eng.call_alleles_by_sequence(sg, win, calls, **dict(args, max_dist=300, min_gain=200))
    swapped, locus_swapped = case["read"].copy(), case["locus"].copy()
    swapped[[4, 5]], locus_swapped[[4, 5]] = swapped[[5, 4]], locus_swapped[[5, 4]]
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: row 5 is out of order"):
        eng.call_alleles_by_sequence(SimpleNamespace(n_loci=sg.n_loci, read=_dev(eng, swapped), locus=_dev(eng, locus_swapped)), win, calls, **args)
    lost = case["sup_read"].copy()
    lost[7] = int(case["read"].max()) + 1
    with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: support entry 7 \(read \d+\) has no row"):
        eng.call_alleles_by_sequence(sg, win, SimpleNamespace(support_off=calls.support_off, read=_dev(eng, lost), value=calls.value), **args)
    off = case["support_off"].copy()
    off[3] = off[4] + 1
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: locus [23]: support_off does not ascend"):
        eng.call_alleles_by_sequence(sg, win, SimpleNamespace(support_off=_dev(eng, off), read=calls.read, value=calls.value), **args)
    assert _raw(eng, case, prm, value=False)[0] == "MTR_ERR_BAD_ARG" and "an input column is NULL" in eng.lib.mtr_last_error(eng.h).decode()
    # short capacities and a NULL column: nothing is written; then the copy succeeds
    m, S, P = case["n_loci"], len(case["sup_read"]), len(want[-1])
    assert _raw(eng, case, prm)[:3] == ("MTR_OK", S, P)
    cols = _dst_columns(eng, m, S, P)
    ptrs = [c.data_ptr() for c in cols]
    torch.cuda.synchronize()
    copy = lambda *a: mtr_amd.STATUS[eng.lib.mtr_call_alleles_sequence_copy_device(eng.h, C.byref(mtr_amd.CSeqCallsDst(*a)))]      # noqa: E731
    for caps in ((m - 1, S, P), (m, S - 1, P), (m, S, P - 1)):
        assert copy(*ptrs, *caps) == "MTR_ERR_OVERFLOW"
    for k in range(13):
        assert copy(*ptrs[:k], None, *ptrs[k + 1:], m, S, P) == "MTR_ERR_BAD_ARG", ref.COLUMNS[k]
    assert mtr_amd.STATUS[eng.lib.mtr_call_alleles_sequence_copy_device(eng.h, None)] == "MTR_ERR_BAD_ARG"
    assert all((c == 77).all() for c in cols)
    assert copy(*ptrs, m, S, P) == "MTR_OK"
    _assert_calls(cols, want, "after the refusals")


# ---- from reads: two alleles of one length -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sc.EQUAL_SEEDS)
def test_two_alleles_of_one_length_from_reads_to_their_sequences(eng, seed):
    reads, loci, truth = sc.equal_reads(seed), cc.truth_loci(), sc.equal_alleles()
    n = 2 * sc.EQUAL_READS
    eng.upload(reads)
    sg = eng.genotype_catalog(loci, 1)
    win = eng.genotype_windows(sg)
    assert sg.read.cpu().tolist() == list(range(n)) and sg.locus.cpu().tolist() == [0] * n
    flat = [sc.equal_windows(seed)[k % 2][k // 2] for k in range(n)]
    assert win.off.cpu().tolist() == list(range(0, 60 * n + 1, 60)) and win.bases.cpu().numpy().tolist() == np.concatenate(flat).tolist()
    calls = eng.call_alleles(sg, "bases")
    assert calls.zygosity.cpu().tolist() == [1, 0] and calls.read.cpu().tolist() == list(range(n))          # one length: one allele by value
    got = eng.call_alleles_by_sequence(sg, win, calls)
    assert got.calls.zygosity.cpu().tolist() == [2, 0] and got.calls.call_support.cpu().tolist() == [[sc.EQUAL_READS] * 2, [0, 0]]
    sides = [r % 2 for r in got.calls.read.cpu().tolist()]                            # read 2 k + a is allele a's
    assert sides == [sides[0]] * sc.EQUAL_READS + [1 - sides[0]] * sc.EQUAL_READS
    assert got.calls.allele.cpu().tolist() == [0] * sc.EQUAL_READS + [1] * sc.EQUAL_READS and got.skipped.cpu().tolist() == [0, 0]
    assert [m % 2 for m in got.medoid.cpu().tolist()[0]] == [sides[0], 1 - sides[0]] and got.medoid.cpu().tolist()[1] == [-1, -1]
    assert got.pair_off.cpu().tolist() == [0, n * (n - 1) // 2, n * (n - 1) // 2]
    case = sc.equal_case(seed)                                                        # the same windows in the same list order: the reference's columns (its reads are numbered otherwise)
    want = dict(zip(ref.COLUMNS, ref.sequence_calls(case, sc.DEFAULT)))
    for name, col in (("dist", got.dist), ("dist_to_medoid", got.dist_to_medoid), ("allele", got.calls.allele), ("cost", got.calls.cost[:1]), ("call_support", got.calls.call_support[:1])):
        assert np.array_equal(col.cpu().numpy(), want[name]), name
    cons = eng.allele_consensus(sg, win, got.calls, band_extra=8)
    off = cons.off.cpu().tolist()
    for a in (0, 1):
        assert cons.bases[off[a]:off[a + 1]].cpu().tolist() == truth[a ^ sides[0]].tolist(), (seed, a)
    text = mtr_amd.format_sequence_calls(loci, got).decode().splitlines()
    assert len(text) == 2 and text[0].split("\t")[:7] == ["0", str(n), "2", "60", "60", "9", "9"] and text[1].split("\t")[-4:] == ["-1", "0/0", "-1", "0/0"]
    assert mtr_amd.format_allele_calls(loci, got.calls).decode().splitlines()[0] == "\t".join(text[0].split("\t")[:-4])
