"""mTR's -a alignments on the device (mtr_report_alignments_device, Engine.report_alignment_tensors, the kernels of
mtr_amd/csrc/report_align.hip.inc) on the MI355X.

Truth is (i) the unmodified reference's recorded -a output, byte for byte, for every golden case that has one and for the file-order
case, and (ii) on whole batches the product's host route: mtr_alignments on mtr_records rebuilt from fetch(), its paths reversed, and
the Python port of print.c's alignment_block for the rows."""
import ctypes as C
import os

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu
from tests.test_gpu_parity import CROWDED_AT, crowded_batch, slots_of
from tests.test_report_align_format import alignment_block_port

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

A_CASES = [name for name, _ in gu.cases("default") if os.path.exists(os.path.join(gu.GOLDEN, f"{name}.a.stdout"))]


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


def _check_shapes(rep, al):
    R = rep.read.numel()
    assert al.col_off.dtype == torch.int64 and al.col_off.shape == (R + 1,) and al.first.shape == (R, 2) and al.first.dtype == torch.int32
    Cn = int(al.col_off[-1]) if R else 0
    assert al.ops.shape == (Cn,) and al.text.shape == (3, Cn) and al.ops.dtype == al.text.dtype == torch.uint8
    assert all(t.device.type == "cuda" for t in al)
    assert int(al.col_off[0]) == 0 and bool((al.col_off[1:] >= al.col_off[:-1]).all())


def test_the_golden_cases_with_recorded_alignments_are_all_here():
    assert len(A_CASES) >= 18 and {"edge", "synth_c2", "synth_c3"} <= set(A_CASES), A_CASES
    assert gu.cases("a") == []                                   # -a has no capture file: the selection above is tests/test_host_driver.py's


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", A_CASES)
def test_golden_cases_print_the_reference_a_stdout(eng, name):
    ids, reads, cut = _golden_reads(name)
    assert not cut, name
    eng.upload(reads)
    eng.run()
    rep = eng.report_tensors()
    al = eng.report_alignment_tensors()
    _check_shapes(rep, al)
    want = open(os.path.join(gu.GOLDEN, f"{name}.a.stdout"), "rb").read()
    assert mtr_amd.format_report(ids, [len(r) for r in reads], rep, alignments=al) == want


def test_file_order_mode_prints_the_stale_base(eng):
    """a repeat that ends on the base an earlier, longer read left behind the read's end: the top row shows that base, not 'A'"""
    recs = gu.read_fasta(os.path.join(gu.GOLDEN, "file_order", "stale_org_base.fa"))
    ids, reads = [h for h, _ in recs], [c for _, c in recs]
    fs = mtr_amd.FileState()
    try:
        eng.upload(reads, fs)
        eng.run()
        rep = eng.report_tensors()
        al = eng.report_alignment_tensors()
    finally:
        fs.close()
    _check_shapes(rep, al)
    want = open(os.path.join(gu.GOLDEN, "file_order", "stale_org_base.a.stdout"), "rb").read()
    assert mtr_amd.format_report(ids, [len(r) for r in reads], rep, alignments=al) == want
    f, lens = rep.fields.cpu().numpy(), np.array([len(r) for r in reads])
    assert (f[:, 1] >= lens[rep.read.cpu().numpy()]).any()        # the case is what it says: a repeat ends behind its read's last base


def test_reads_given_as_device_text(eng):
    """upload_device: the host never packs the bases; the same bytes come out"""
    ids, reads, _ = _golden_reads("synth_c2")
    eng.upload_device(*_ascii_tensor(reads))
    eng.run()
    rep = eng.report_tensors()
    al = eng.report_alignment_tensors()
    want = open(os.path.join(gu.GOLDEN, "synth_c2.a.stdout"), "rb").read()
    assert mtr_amd.format_report(ids, [len(r) for r in reads], rep, alignments=al) == want


def _host_alignments(e, rep, got):
    """the product's host route: mtr_records of the chain's records from fetch(), mtr_alignments -> (ops, off, end) as numpy"""
    read, record = rep.read.cpu().numpy(), rep.record.cpu().numpy()
    R = len(read)
    recs = (mtr_amd.CRecord * max(R, 1))()
    for k in range(R):
        g, r = got[int(read[k])][int(record[k])], recs[k]
        (r.rep_start, r.rep_end, r.repeat_len, r.rep_period, r.num_freq_unit, r.num_matches, r.num_mismatches, r.num_insertions,
         r.num_deletions, r.kmer, r.match_gain, r.mismatch_penalty, r.indel_penalty) = g[:13]
        r.unit = g.unit.encode()
    rd = np.ascontiguousarray(read, np.int32)
    po, pf, pe = C.POINTER(C.c_uint8)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
    e._check(e.lib.mtr_alignments(e.h, R, rd.ctypes.data_as(C.POINTER(C.c_int32)), recs, C.byref(po), C.byref(pf), C.byref(pe)), "mtr_alignments")
    try:
        off = np.ctypeslib.as_array(pf, shape=(R + 1,)).copy()
        end = np.ctypeslib.as_array(pe, shape=(max(R, 1), 2))[:R].copy()
        ops = np.ctypeslib.as_array(po, shape=(max(int(off[-1]), 1),))[:int(off[-1])].copy()
    finally:
        for p in (po, pf, pe):
            mtr_amd._libc.free(C.cast(p, C.c_void_p))
    return ops, off, end


BATCHES = [("headline2k", 10000, False), ("headline2k", 10000, True), ("c4", 10000, False)]


def _check_against_the_host_route(e, reads, got, rep, al):
    """every repeat of the batch: the device's columns are mtr_alignments' path reversed, first is its end walked back through the
    path, and the three rows are what alignment_block prints for that path.  Returns the number of repeats."""
    _check_shapes(rep, al)
    h_ops, h_off, h_end = _host_alignments(e, rep, got)
    col_off, ops, text, first = (t.cpu().numpy() for t in al)
    read, fields = rep.read.cpu().numpy(), rep.fields.cpu().numpy()
    unit_off, units = rep.unit_off.cpu().numpy(), rep.units.cpu().numpy().tobytes()
    R = len(read)
    assert np.array_equal(col_off, h_off)                          # same lengths, repeat for repeat
    compared = 0
    for k in range(R):
        c0, c1 = int(col_off[k]), int(col_off[k + 1])
        tb = h_ops[c0:c1]
        assert c1 > c0 and np.array_equal(ops[c0:c1], tb[::-1]), k
        U = int(fields[k, 3])
        p_first = int(h_end[k, 0]) - int((tb[:-1] != 3).sum())
        j_first = (int(h_end[k, 1]) - 1 - int((tb[:-1] != 4).sum())) % U + 1
        assert first[k].tolist() == [p_first, j_first], (k, first[k].tolist(), p_first, j_first)
        rd = int(read[k])
        block = alignment_block_port(reads[rd], len(reads[rd]), (0, 0), fields[k].tolist(), units[unit_off[k]:unit_off[k + 1]], tb.tolist(),
                                     int(h_end[k, 0]), int(h_end[k, 1]))
        body = block.split(b"\n")[3:]
        for r in range(3):
            assert text[r, c0:c1].tobytes() == b"".join(body[r::4]), (k, r)
        compared += 1
    assert compared == R
    return R


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("cfg,n,pearson", BATCHES, ids=[f"{c}_{n}{'_p' if p else ''}" for c, n, p in BATCHES])
def test_whole_batches_against_the_host_route(eng, eng_p, cfg, n, pearson):
    reads = [c for _, c in synth.make_reads(cfg, n, synth.CONFIGS[cfg][4])]
    e = eng_p if pearson else eng
    e.upload(reads)
    e.run()
    got = e.fetch()
    rep = e.report_tensors()
    al = e.report_alignment_tensors()
    assert _check_against_the_host_route(e, reads, got, rep, al) > n // 2
    assert np.array_equal(np.unique(al.ops.cpu().numpy()), [1, 2, 3, 4])


@pytest.mark.parametrize("where", list(CROWDED_AT))
def test_a_read_with_more_records_than_slots(eng, where):
    """the crowded read's records are read through the pointer table (resolve_overflow), as the first, a middle and the last read;
    mtr_alignments takes the records the caller gives it, so the host route does not go through that table"""
    reads, i = crowded_batch(where)
    eng.upload(reads)
    eng.run()
    got = eng.fetch()
    assert len(got[i]) > slots_of(reads)
    rep = eng.report_tensors()
    assert _check_against_the_host_route(eng, reads, got, rep, eng.report_alignment_tensors()) >= int(rep.counts[i]) > 0


def test_protocol(monkeypatch):
    lib = mtr_amd.load_library()
    e = mtr_amd.Engine()
    try:
        R, Cn = C.c_int64(-1), C.c_int64(-1)
        assert lib.mtr_report_alignments_device(e.h, None, C.byref(R), C.byref(Cn)) == 2           # before any upload: MTR_ERR_BAD_ARG
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
            e.report_alignment_tensors()
        reads = [c for _, c in synth.make_reads("headline2k", 200, 3)]
        e.upload(reads)
        assert lib.mtr_report_alignments_device(e.h, None, C.byref(R), C.byref(Cn)) == 2           # uploaded, not run
        e.run()
        # without a prior mtr_report_device: the call makes the chains itself
        assert lib.mtr_report_alignments_device(e.h, None, C.byref(R), C.byref(Cn)) == 0
        assert R.value > 0 and Cn.value > R.value
        rep = e.report_tensors()
        assert rep.read.numel() == R.value
        al = e.report_alignment_tensors()
        _check_shapes(rep, al)
        assert al.ops.numel() == Cn.value
        f, co = rep.fields.cpu().numpy(), al.col_off.cpu().numpy()
        gaps = np.bincount(np.repeat(np.arange(R.value), np.diff(co)), weights=al.ops.cpu().numpy() == 3, minlength=R.value)
        bases = np.diff(co) - gaps                                  # columns that hold a read base: within the repeat's window
        assert (bases >= 1).all() and (bases <= f[:, 1] - f[:, 0] + 1).all()
        p0 = al.first.cpu().numpy()[:, 0]
        assert (p0 >= f[:, 0]).all() and (p0 + bases - 1 <= f[:, 1]).all()
        # capacities one short: MTR_ERR_OVERFLOW with the sizes, nothing written
        dev = torch.device("cuda", 0)
        col_off = torch.full((R.value + 1,), -7, dtype=torch.int64, device=dev)
        ops = torch.full((Cn.value,), 99, dtype=torch.uint8, device=dev)
        text = torch.full((3, Cn.value), 99, dtype=torch.uint8, device=dev)
        first = torch.full((R.value, 2), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for cap_r, cap_c in ((R.value - 1, Cn.value), (R.value, Cn.value - 1)):
            dst = mtr_amd.CReportAlignDst(col_off.data_ptr(), ops.data_ptr(), text.data_ptr(), first.data_ptr(), cap_r, cap_c)
            R2, C2 = C.c_int64(), C.c_int64()
            assert lib.mtr_report_alignments_device(e.h, C.byref(dst), C.byref(R2), C.byref(C2)) == 5      # MTR_ERR_OVERFLOW
            assert (R2.value, C2.value) == (R.value, Cn.value)
            torch.cuda.synchronize()
            assert bool((col_off == -7).all()) and bool((ops == 99).all()) and bool((text == 99).all()) and bool((first == -7).all())
        # exact capacities into the poisoned tensors; a second call gives identical tensors
        dst = mtr_amd.CReportAlignDst(col_off.data_ptr(), ops.data_ptr(), text.data_ptr(), first.data_ptr(), R.value, Cn.value)
        assert lib.mtr_report_alignments_device(e.h, C.byref(dst), C.byref(R), C.byref(Cn)) == 0
        again = e.report_alignment_tensors()
        for a, b, c in zip(al, again, (col_off, ops, text, first)):
            assert torch.equal(a, b) and torch.equal(a, c) and a.data_ptr() != b.data_ptr()
        assert int(ops.max()) <= 4 and int(ops.min()) >= 1
        # mtr_alignments (the command line's route) in between does not disturb the kept alignments
        got = e.fetch()
        _host_alignments(e, rep, got)
        for a, b in zip(al, e.report_alignment_tensors()):
            assert torch.equal(a, b)
        # a new upload invalidates it; a new run gives the new batch's alignments
        e.upload(reads[:50])
        assert lib.mtr_report_alignments_device(e.h, None, C.byref(R), C.byref(Cn)) == 2
        e.run()
        part = e.report_alignment_tensors()
        n50 = int(rep.counts[:50].sum())
        c50 = int(al.col_off[n50])
        assert part.first.shape[0] == n50 and torch.equal(part.ops, al.ops[:c50]) and torch.equal(part.text, al.text[:, :c50])
        assert torch.equal(part.col_off, al.col_off[:n50 + 1]) and torch.equal(part.first, al.first[:n50])
        # reads that report nothing: R = 0, C = 0
        e.upload([np.zeros(100, np.uint8)])                        # a homopolymer: mTR reports nothing (edge.fa)
        e.run()
        assert lib.mtr_report_alignments_device(e.h, None, C.byref(R), C.byref(Cn)) == 0 and (R.value, Cn.value) == (0, 0)
        empty = e.report_alignment_tensors()
        assert empty.col_off.cpu().tolist() == [0] and empty.ops.numel() == 0 and empty.text.shape == (3, 0) and empty.first.shape == (0, 2)
        assert mtr_amd.format_report(["x"], [100], e.report_tensors(), alignments=empty) == b""
    finally:
        e.close()


def test_a_run_that_failed_answers_with_its_status(monkeypatch):
    """MTR_ERR_DP_TOO_LARGE latched by the run (the batch and the lowered WrapDPsize of tests/test_gpu_parity.py: a documented error
    path, read by mtr_create): the alignments call returns that status, as mtr_report_device does"""
    from tests.test_gpu_parity import WRAP_LIMIT
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(WRAP_LIMIT))
    rng = np.random.RandomState(60)
    small = [rng.randint(0, 4, size=n).astype(np.uint8) for n in (700, 1500)] + [np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 60)]
    small += [synth.make_read(rng, 12, 14, 100, 100)[0], synth.make_read(rng, 30, 9, 50, 300)[0]]
    big = [c for _, c in synth.make_reads("headline2k", 6, 61)]
    reads = small + big[:3] + small[:2] + big[3:]
    e = mtr_amd.Engine()
    try:
        e.upload(reads)
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
            e.run()
        R, Cn = C.c_int64(), C.c_int64()
        assert e.lib.mtr_report_alignments_device(e.h, None, C.byref(R), C.byref(Cn)) == 6            # MTR_ERR_DP_TOO_LARGE
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
            e.report_alignment_tensors()
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
            e.report_tensors()
        # the reads below the limit alone run clean on the same context and are aligned
        e.upload(small)
        e.run()
        al = e.report_alignment_tensors()
        assert al.first.shape[0] == e.report_tensors().read.numel() > 0
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                                   # mtr_create puts the built-in limit back on the device
