"""mTR's stdout on the device (mtr_report_text_device, Engine.report_text / report_bytes, the kernels of
mtr_amd/csrc/report_text.hip.inc) on the MI355X.

Truth is (i) the unmodified reference's recorded stdout, byte for byte, plain and -a, with no Python formatter between the device and
the comparison; (ii) the sha256 known answers of whole batches; (iii) on whole -a batches and on the fuzz rows mtr_amd.format_report,
which tests/test_report_format.py and tests/test_report_text_format.py pin to print.c and to glibc."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu
from tests import host_util as hu
from tests.test_gpu_parity import CROWDED_AT, crowded_batch, slots_of
from tests.test_report_text_format import INT_MAX, INT_MIN, PINNED, fuzz_report, fuzz_rows

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

A_CASES = [name for name, _ in gu.cases("default") if os.path.exists(os.path.join(gu.GOLDEN, f"{name}.a.stdout"))]     # tests/test_gpu_report_align.py's selection


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_p():
    e = mtr_amd.Engine(manhattan=False)
    yield e
    e.close()


def _golden_reads(name):
    """(ids, codes) of the reads mTR reports: the FASTA's records up to its first empty one (the reference stops there)"""
    recs, hdr, seq = [], None, []
    with open(gu.input_path(name)) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if hdr is not None:
                    recs.append((hdr, "".join(seq)))
                hdr, seq = line[1:], []
            else:
                seq.append(line)
    if hdr is not None:
        recs.append((hdr, "".join(seq)))
    cut = next((i for i, (_, s) in enumerate(recs) if not s), len(recs))
    return [h for h, _ in recs[:cut]], [mtr_amd.codes_from_str(s) for _, s in recs[:cut]], cut < len(recs)


def _ascii_tensor(reads):
    text = np.concatenate([np.frombuffer(b"ACGT", np.uint8)[r] for r in reads])
    lens = np.array([len(r) for r in reads], np.int32)
    offs = np.zeros(len(reads), np.int64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    return torch.from_numpy(text).to("cuda:0"), offs, lens


def _one_read(rep, al, i):
    """the Report (and ReportAlignments) of read i alone, as numpy columns"""
    counts = rep.counts.numpy()
    k0 = int(counts[:i].sum())
    k1 = k0 + int(counts[i])
    uo = rep.unit_off.cpu().numpy()
    sub = mtr_amd.Report(counts[i:i + 1], np.full(k1 - k0, i, np.int32), rep.record.cpu().numpy()[k0:k1], rep.fields.cpu().numpy()[k0:k1],
                         rep.ratio.cpu().numpy()[k0:k1], uo[k0:k1 + 1] - uo[k0], rep.units.cpu().numpy()[uo[k0]:uo[k1]])
    if al is None:
        return sub, None
    co = al.col_off.cpu().numpy()
    return sub, mtr_amd.ReportAlignments(co[k0:k1 + 1] - co[k0], al.ops.cpu().numpy()[co[k0]:co[k1]], al.text.cpu().numpy()[:, co[k0]:co[k1]],
                                         al.first.cpu().numpy()[k0:k1])


def _check_text(e, ids, reads, alignments, want):
    """report_bytes is `want`; report_text's tensors have their shapes, and read_off cuts the text where format_report of each read does"""
    assert e.report_bytes(ids, alignments=alignments) == want
    rt = e.report_text(ids, alignments=alignments)
    n = len(reads)
    assert rt.text.dtype == torch.uint8 and rt.text.shape == (len(want),) and rt.read_off.dtype == torch.int64 and rt.read_off.shape == (n + 1,)
    assert rt.text.device.type == rt.read_off.device.type == "cuda"
    text, off = rt.text.cpu().numpy().tobytes(), rt.read_off.cpu().tolist()
    assert text == want and off[0] == 0 and off[-1] == len(want)
    rep = e.report_tensors()
    al = e.report_alignment_tensors() if alignments else None
    lens = [len(r) for r in reads]
    for i in range(n):
        sub, sub_al = _one_read(rep, al, i)
        assert text[off[i]:off[i + 1]] == mtr_amd.format_report(ids, lens, sub, alignments=sub_al), (i, ids[i])


def test_the_golden_cases_with_recorded_alignments_are_all_here():
    assert len(A_CASES) >= 18 and {"edge", "synth_c2", "synth_c3"} <= set(A_CASES), A_CASES


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,mode", gu.cases("default") + gu.cases("p"))
def test_golden_cases_print_the_reference_stdout(eng, eng_p, name, mode):
    e = eng if mode == "default" else eng_p
    ids, reads, cut = _golden_reads(name)
    assert not cut, name
    e.upload(reads)
    e.run()
    _check_text(e, ids, reads, False, open(os.path.join(gu.GOLDEN, f"{name}.{mode}.stdout"), "rb").read())


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", A_CASES)
def test_golden_cases_print_the_reference_a_stdout(eng, name):
    ids, reads, cut = _golden_reads(name)
    assert not cut, name
    eng.upload(reads)
    eng.run()
    _check_text(eng, ids, reads, True, open(os.path.join(gu.GOLDEN, f"{name}.a.stdout"), "rb").read())


def test_file_order_mode_prints_the_stale_base(eng):
    """a repeat that ends on the base an earlier, longer read left behind the read's end: the top row shows that base, not 'A'"""
    recs = gu.read_fasta(os.path.join(gu.GOLDEN, "file_order", "stale_org_base.fa"))
    ids, reads = [h for h, _ in recs], [c for _, c in recs]
    fs = mtr_amd.FileState()
    try:
        eng.upload(reads, fs)
        eng.run()
        want = open(os.path.join(gu.GOLDEN, "file_order", "stale_org_base.a.stdout"), "rb").read()
        _check_text(eng, ids, reads, True, want)
        rep = eng.report_tensors()
    finally:
        fs.close()
    f, lens = rep.fields.cpu().numpy(), np.array([len(r) for r in reads])
    assert (f[:, 1] >= lens[rep.read.cpu().numpy()]).any()        # the case is what it says: a repeat ends behind its read's last base


def test_reads_given_as_device_text(eng):
    """upload_device: the host never packs the bases, and never sees the report before it is text"""
    ids, reads, _ = _golden_reads("synth_c2")
    eng.upload_device(*_ascii_tensor(reads))
    eng.run()
    assert eng.report_bytes(ids, alignments=True) == open(os.path.join(gu.GOLDEN, "synth_c2.a.stdout"), "rb").read()
    assert eng.report_bytes(ids) == open(os.path.join(gu.GOLDEN, "synth_c2.default.stdout"), "rb").read()


KNOWN = [("headline2k", 10000, False), ("headline2k", 10000, True), ("c2", 1000, False), ("c4", 10000, False)]      # tests/test_gpu_report.py::KNOWN


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg,n,pearson", KNOWN, ids=[f"{c}_{n}{'_p' if p else ''}" for c, n, p in KNOWN])
def test_whole_batches_match_their_known_answers(eng, eng_p, cfg, n, pearson):
    known = hu.load_known(f"{cfg}_{n}{'_p' if pearson else ''}_stdout.json")
    reads = [c for _, c in synth.make_reads(cfg, n, synth.CONFIGS[cfg][4])]
    e = eng_p if pearson else eng
    e.upload(reads)
    e.run()
    out = e.report_bytes([str(i) for i in range(n)])
    assert (hashlib.sha256(out).hexdigest(), out.count(b"\n"), len(out)) == (known["sha256"], known["stdout_lines"], known["stdout_bytes"])


A_BATCHES = [("headline2k", 10000), ("c4", 10000)]


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("cfg,n", A_BATCHES, ids=[f"{c}_{n}" for c, n in A_BATCHES])
def test_whole_batches_with_alignments_equal_format_report(eng, cfg, n):
    reads = [c for _, c in synth.make_reads(cfg, n, synth.CONFIGS[cfg][4])]
    ids = [str(i) for i in range(n)]
    eng.upload(reads)
    eng.run()
    out = eng.report_bytes(ids, alignments=True)
    rep = eng.report_tensors()
    al = eng.report_alignment_tensors()
    cols = np.diff(al.col_off.cpu().numpy())
    assert len(cols) > n // 2
    assert ((cols > 0) & (cols % mtr_amd.ALIGN_WIDTH == 0)).any() and (cols % mtr_amd.ALIGN_WIDTH != 0).any()      # a full last block, and a narrower one
    want = mtr_amd.format_report(ids, [len(r) for r in reads], rep, alignments=al)
    assert len(out) == len(want) and hashlib.sha256(out).digest() == hashlib.sha256(want).digest() and out == want
    off = eng.report_text(ids, alignments=True).read_off.cpu().numpy()
    counts = rep.counts.numpy()
    assert off[0] == 0 and off[-1] == len(out) and (np.diff(off) > 0).tolist() == (counts > 0).tolist()


@pytest.mark.parametrize("where", list(CROWDED_AT))
def test_a_read_with_more_records_than_slots(eng, where):
    """the crowded read's records are read through the pointer table (resolve_overflow), as the first, a middle and the last read"""
    reads, i = crowded_batch(where)
    ids = [f"read{k}" for k in range(len(reads))]
    eng.upload(reads)
    eng.run()
    assert len(eng.fetch()[i]) > slots_of(reads)
    rep = eng.report_tensors()
    assert int(rep.counts[i]) > 0
    lens = [len(r) for r in reads]
    _check_text(eng, ids, reads, False, mtr_amd.format_report(ids, lens, rep))
    _check_text(eng, ids, reads, True, mtr_amd.format_report(ids, lens, rep, alignments=eng.report_alignment_tensors()))


def _every_answer(e, ids):
    """what every call that reads the finished batch returns, as comparable values"""
    texts = [e.report_text(ids, alignments=True) for _ in range(2)]
    rep = e.report_tensors()
    data, counts = e.fetch_packed()
    return ([(t.text.cpu().numpy().tobytes(), t.read_off.cpu().tolist()) for t in texts],
            [rep.counts.tolist()] + [c.cpu().numpy().tobytes() for c in rep[1:]], data, counts.tolist(), e.fetch())


@pytest.mark.parametrize("where", list(CROWDED_AT))
def test_the_pointer_table_is_made_once_per_run(eng, where):
    """the table of the crowded batch is made when its run ends: every reading call after it, in any order and repeated, and the same
    calls after the resident batch ran once more, give the same bytes (a stale or dangling table would not)"""
    reads, i = crowded_batch(where)
    ids = [f"read{k}" for k in range(len(reads))]
    eng.upload(reads)
    eng.run()
    first = _every_answer(eng, ids)
    assert len(first[4][i]) > slots_of(reads)
    assert first[0][0] == first[0][1]
    assert first[0][0][0] == mtr_amd.format_report(ids, [len(r) for r in reads], eng.report_tensors(), alignments=eng.report_alignment_tensors())
    eng.run()
    assert _every_answer(eng, ids) == first


def test_formatter_fuzz(eng):
    """mtr_test_report_lines (the same device function) on seeded rows against format_report of the same rows: every row is compared"""
    fields, read_len, units, ids = fuzz_rows()
    n = len(fields)
    assert n >= 3000
    flat = set(fields.ravel().tolist()) | set(read_len.tolist())
    assert {0, INT_MIN, INT_MAX} <= flat and any(v < 0 for v in flat)
    assert {0, 1, 499} <= {len(u) for u in units} and any(len(i) == 0 for i in ids) and any(len(i) >= 300 for i in ids)
    got = eng.test_report_lines(fields, read_len, units, ids)
    assert len(got) == n
    want = mtr_amd.format_report(ids, read_len, fuzz_report(fields, units))
    lines = want.split(b"\n")
    assert len(lines) == n + 1 and lines[-1] == b""
    bad = [k for k in range(n) if got[k] != lines[k] + b"\n"]
    assert not bad, f"{len(bad)} of {n} rows differ; first: row {bad[0]}: {got[bad[0]]!r} != {lines[bad[0]]!r}"
    assert b"".join(got) == want
    for k, (_, _, text) in enumerate(PINNED):
        assert got[k].split(b"\t")[-5] == text.encode(), (PINNED[k], got[k])
    assert eng.test_report_lines(np.zeros((0, 14), np.int32), [], [], []) == []


def _call(e, data, off, mode, dst, nb):
    return e.lib.mtr_report_text_device(e.h, data.ctypes.data if data is not None else None, off.ctypes.data if off is not None else None, mode,
                                        C.byref(dst) if dst is not None else None, C.byref(nb))


def test_protocol():
    e = mtr_amd.Engine()
    try:
        nb = C.c_int64(-1)
        data, off = mtr_amd.pack_ids([])
        assert _call(e, data, off, 0, None, nb) == 2                  # before any upload: MTR_ERR_BAD_ARG
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
            e.report_text([])
        reads = [c for _, c in synth.make_reads("headline2k", 200, 3)]
        ids = [f"read {i}/x" if i % 5 else "" for i in range(len(reads))]
        lens = [len(r) for r in reads]
        data, off = mtr_amd.pack_ids(ids)
        e.upload(reads)
        assert _call(e, data, off, 0, None, nb) == 2                  # uploaded, not run
        with pytest.raises(mtr_amd.MtrError, match="199 ids for 200"):
            e.report_text(ids[:-1])
        e.run()
        # a sizes-only call, first with alignments and with no report call before it: it makes the chains and the alignments itself
        sizes = {}
        for mode in (1, 0):
            assert _call(e, data, off, mode, None, nb) == 0
            sizes[mode] = nb.value
        assert 0 < sizes[0] < sizes[1]
        assert _call(e, None, off, 0, None, nb) == 2 and b"NULL" in e.lib.mtr_last_error(e.h)
        assert _call(e, data, None, 0, None, nb) == 2
        bad_off = off.copy()
        bad_off[7] = bad_off[8] + 1
        assert _call(e, data, bad_off, 0, None, nb) == 2 and b"id_off" in e.lib.mtr_last_error(e.h)
        # the oracle by the columns: both modes, asked one after the other and again
        text_a = e.report_bytes(ids, alignments=True)
        text_p = e.report_bytes(ids)
        al = e.report_alignment_tensors()
        rep = e.report_tensors()
        assert text_p == mtr_amd.format_report(ids, lens, rep) and len(text_p) == sizes[0]
        assert text_a == mtr_amd.format_report(ids, lens, rep, alignments=al) and len(text_a) == sizes[1]
        assert e.report_bytes(ids, alignments=True) == text_a and e.report_bytes(ids) == text_p
        dev = torch.device("cuda", 0)
        for mode, want in ((0, text_p), (1, text_a)):
            B = len(want)
            # one byte short: MTR_ERR_OVERFLOW with the size, nothing written
            text = torch.full((B,), 0x7e, dtype=torch.uint8, device=dev)
            read_off = torch.full((len(reads) + 1,), -7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            dst = mtr_amd.CReportTextDst(text.data_ptr(), read_off.data_ptr(), B - 1)
            nb.value = -1
            assert _call(e, data, off, mode, dst, nb) == 5 and nb.value == B
            torch.cuda.synchronize()
            assert bool((text == 0x7e).all()) and bool((read_off == -7).all())
            # the exact capacity, into the marked memory; then without read_off
            dst = mtr_amd.CReportTextDst(text.data_ptr(), read_off.data_ptr(), B)
            assert _call(e, data, off, mode, dst, nb) == 0 and nb.value == B
            assert text.cpu().numpy().tobytes() == want
            ro = read_off.cpu().tolist()
            assert ro[0] == 0 and ro[-1] == B and all(a <= b for a, b in zip(ro, ro[1:]))
            text.fill_(0x7e)
            torch.cuda.synchronize()
            dst = mtr_amd.CReportTextDst(text.data_ptr(), None, B)
            assert _call(e, data, off, mode, dst, nb) == 0 and text.cpu().numpy().tobytes() == want
        # the other orders after a fresh run: the columns first, the text behind them; the text between the two column calls
        e.run()
        rep2 = e.report_tensors()
        assert e.report_bytes(ids) == text_p
        al2 = e.report_alignment_tensors()
        assert e.report_bytes(ids, alignments=True) == text_a and e.report_bytes(ids) == text_p
        for a, b in zip(list(rep)[1:] + list(al), list(rep2)[1:] + list(al2)):
            assert torch.equal(a, b)
        e.run()
        al3 = e.report_alignment_tensors()
        assert e.report_bytes(ids, alignments=True) == text_a
        for a, b in zip(al, al3):
            assert torch.equal(a, b)
        # a new upload invalidates it; a new run gives the new batch's text, which is the first reads' part of the old one
        e.upload(reads[:50])
        data50, off50 = mtr_amd.pack_ids(ids[:50])
        assert _call(e, data50, off50, 1, None, nb) == 2
        e.run()
        part = e.report_bytes(ids[:50], alignments=True)
        assert part and text_a.startswith(part)
        # reads that report nothing: B = 0, read_off all zero
        e.upload([np.zeros(100, np.uint8), np.zeros(150, np.uint8)])   # homopolymers: mTR reports nothing (edge.fa)
        e.run()
        for alignments in (False, True):
            empty = e.report_text(["x", "y"], alignments=alignments)
            assert empty.text.numel() == 0 and empty.read_off.cpu().tolist() == [0, 0, 0]
            assert e.report_bytes(["x", "y"], alignments=alignments) == b""
    finally:
        e.close()


def test_a_run_that_failed_answers_with_its_status(monkeypatch):
    """MTR_ERR_DP_TOO_LARGE latched by the run (the batch and the lowered WrapDPsize of tests/test_gpu_parity.py: a documented error
    path, read by mtr_create): the text call returns that status, as mtr_report_device does"""
    from tests.test_gpu_parity import WRAP_LIMIT
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(WRAP_LIMIT))
    rng = np.random.RandomState(60)
    small = [rng.randint(0, 4, size=n).astype(np.uint8) for n in (700, 1500)] + [np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 60)]
    small += [synth.make_read(rng, 12, 14, 100, 100)[0], synth.make_read(rng, 30, 9, 50, 300)[0]]
    big = [c for _, c in synth.make_reads("headline2k", 6, 61)]
    reads = small + big[:3] + small[:2] + big[3:]
    ids = [str(i) for i in range(len(reads))]
    e = mtr_amd.Engine()
    try:
        e.upload(reads)
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
            e.run()
        nb = C.c_int64()
        data, off = mtr_amd.pack_ids(ids)
        for mode in (0, 1):
            assert _call(e, data, off, mode, None, nb) == 6           # MTR_ERR_DP_TOO_LARGE
        for alignments in (False, True):
            with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
                e.report_text(ids, alignments=alignments)
            with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
                e.report_bytes(ids, alignments=alignments)
        # the reads below the limit alone run clean on the same context and are printed
        e.upload(small)
        e.run()
        sid, lens = ids[:len(small)], [len(r) for r in small]
        text = e.report_bytes(sid, alignments=True)
        assert text and text == mtr_amd.format_report(sid, lens, e.report_tensors(), alignments=e.report_alignment_tensors())
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                                   # mtr_create puts the built-in limit back on the device
