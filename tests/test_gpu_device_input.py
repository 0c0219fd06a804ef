"""Reads in device memory on the MI355X: Engine.upload_device / process_device (mtr_upload_batch_device, the packing kernel
mtr_k_pack_text) give the records and wire bytes of the host path on the same reads, for ASCII and code text, either case,
reads at unaligned offsets between junk bytes, text written by torch on the current stream just before the call; bad input
is refused and leaves the engine usable; export_tensor and the -a alignments close the round trip on the device."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
JUNK_ASCII = np.frombuffer(b"N\n\xff>n-", np.uint8)
JUNK_CODES = np.array([4, 0xFF, ord("N"), ord("\n"), 7], np.uint8)


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


def _text(reads, codes=False, lower=0.0, junk=False, seed=0):
    """reads (codes 0..3) -> (text uint8 on the host, offsets int64, lens int32): ASCII (a share `lower` of the bases in lower
    case) or codes; junk=True puts 1..7 bytes that are no base in front of and between the reads (unaligned offsets)"""
    rng = np.random.RandomState(seed)
    parts, offs, at = [], [], 0
    for r in reads:
        if junk:
            j = (JUNK_CODES if codes else JUNK_ASCII)[rng.randint(0, 5, size=rng.randint(1, 8))]
            parts.append(j)
            at += len(j)
        b = np.asarray(r, np.uint8).copy() if codes else ACGT[np.asarray(r, np.uint8)].copy()
        if lower and not codes:
            b[rng.rand(len(b)) < lower] += 32
        parts.append(b)
        offs.append(at)
        at += len(b)
    if junk:
        parts.append(JUNK_ASCII[:3])
    return np.concatenate(parts), np.array(offs, np.int64), np.array([len(r) for r in reads], np.int32)


def _host(e, reads):
    e.upload(reads)
    e.run()
    return e.fetch(), e.fetch_packed()


def _device(e, reads, **kw):
    text, offs, lens = _text(reads, **kw)
    t = torch.from_numpy(text).cuda()
    got = e.process_device(t, offs, lens, codes=kw.get("codes", False))
    return got, e.fetch_packed()


def _same(e, reads, **kw):
    want, (wblob, wcnt) = _host(e, reads)
    got, (gblob, gcnt) = _device(e, reads, **kw)
    assert len(got) == len(want) == len(reads)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a == b, f"read {i} (length {len(reads[i])}): host {len(a)} records, device {len(b)}"
    assert np.array_equal(wcnt, gcnt) and wblob == gblob
    return want


# ---- equality with the host path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", gu.cases())
def test_golden_reads(eng, eng_p, name, mode):
    reads = [c for _, c in gu.read_fasta(gu.input_path(name))]
    _same(eng if mode == "default" else eng_p, reads)


@pytest.mark.parametrize("kw", [{}, {"codes": True}, {"lower": 0.5, "junk": True, "seed": 3}, {"codes": True, "junk": True, "seed": 4}],
                         ids=["ascii", "codes", "mixed_case_junk", "codes_junk"])
def test_headline_shaped_reads(eng, kw):
    reads = [c for _, c in synth.make_reads("headline2k", 2000)]
    want = _same(eng, reads, **kw)
    assert sum(len(w) for w in want) > 2000


@pytest.mark.timeout(900)
def test_full_size_headline_batch_matches_the_known_answer(eng):
    """The whole headline batch (10 000 reads, 20.5 M bases) as ASCII text in a torch tensor: the packing kernel's image feeds the
    default selection at full size, and the record stream is the CPU oracle's (tests/golden/headline2k_10000_wire.json)"""
    from tests import host_util as hu
    from tests.test_gpu_parity import _diff_msg
    reads = [c for _, c in synth.make_reads("headline2k", 10000, synth.CONFIGS["headline2k"][4])]
    got, (blob, counts) = _device(eng, reads)
    assert eng.last_mode() == "staged chain" and eng.counters()["reads_sent_back"] == 0
    assert counts.tolist() == [len(g) for g in got]
    bad = hu.known_wire_mismatch(blob, counts, reads, hu.load_known("headline2k_10000_wire.json"), _diff_msg)
    assert bad is None, bad


def test_config3_shaped_reads(eng):
    reads = [c for _, c in synth.make_reads("c3", 3)]
    _same(eng, reads, lower=1.0, junk=True, seed=5)


@pytest.mark.parametrize("codes", [False, True])
def test_short_reads_of_every_length_mod_16(eng, codes):
    rng = np.random.RandomState(11)
    reads = [rng.randint(0, 4, size=n).astype(np.uint8) for n in range(1, 41)]
    reads += [np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 40)]
    reads += [rng.randint(0, 4, size=int(n)).astype(np.uint8) for n in rng.randint(41, 600, size=60)]
    rng.shuffle(reads)
    _same(eng, reads, codes=codes, junk=True, lower=0.3, seed=12)


def test_read_of_the_maximum_length(eng):
    rng = np.random.RandomState(99)
    parts = []
    for unit_len, copies in ((180, 40), (3, 300), (60, 150)):
        parts.append(rng.randint(0, 4, size=270000).astype(np.uint8))
        parts.append(synth.make_read(rng, unit_len, copies, 0, 0)[0])
    read = np.concatenate(parts)
    read = np.concatenate([read, rng.randint(0, 4, size=mtr_amd.MAX_READ_LENGTH - len(read)).astype(np.uint8)])
    want = _same(eng, [read], junk=True, seed=7)
    assert len(want[0]) > 500


# ---- stream ordering ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side_stream", [False, True])
def test_text_written_by_torch_just_before_the_call(eng, side_stream):
    """the text is made by a lookup on torch's current stream behind a few ms of other work there, with no synchronise:
    the packing kernel must wait for it (an event on that stream)"""
    reads = [c for _, c in synth.make_reads("headline2k", 1000, seed=21)]
    want, (wblob, _) = _host(eng, reads)
    codes, offs, lens = _text(reads, codes=True)
    dev = torch.device("cuda", 0)
    codes_t = torch.from_numpy(codes).to(dev)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev) if side_stream else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        x = torch.randn(4096, 4096, device=dev)
        for _ in range(6):
            x = x @ x / 64.0                                  # (keeps the stream busy)
        text = lut.index_select(0, codes_t.long())
        got = eng.process_device(text, offs, lens)
    assert got == want
    assert eng.fetch_packed()[0] == wblob
    torch.cuda.synchronize()


# ---- bad input ------------------------------------------------------------------------------------------------------------
def test_bad_bytes_name_the_read_and_leave_the_engine_usable(eng):
    reads = [c for _, c in synth.make_reads("c2", 12, seed=31)]
    text, offs, lens = _text(reads, junk=True, seed=32)
    bad = text.copy()
    bad[offs[5] + 17] = ord("N")
    bad[offs[9] + 3] = ord("\n")
    with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: read 5:"):
        eng.upload_device(torch.from_numpy(bad).cuda(), offs, lens)
    with pytest.raises(mtr_amd.MtrError, match="no batch uploaded"):          # nothing is left uploaded
        eng.run()
    ctext, coffs, clens = _text(reads, codes=True)
    ctext[coffs[11] + lens[11] - 1] = 4
    with pytest.raises(mtr_amd.MtrError, match=r"read 11: base code > 3"):
        eng.upload_device(torch.from_numpy(ctext).cuda(), coffs, clens, codes=True)
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):
        eng.upload_device(torch.from_numpy(text), offs, lens)
    o = offs.copy()
    o[3] = len(text) - 5
    with pytest.raises(mtr_amd.MtrError, match="read 3: bytes"):
        eng.upload_device(torch.from_numpy(text).cuda(), o, lens)
    _same(eng, reads, junk=True, seed=33)                                     # the same engine, a good batch


def test_library_refuses_what_the_python_checks_do_not_see(eng):
    """called straight through the C-ABI: host memory, an unknown text_kind, a read outside text_bytes; each is MTR_ERR_BAD_ARG
    with a reason, and the next upload works"""
    lib = eng.lib
    reads = [c for _, c in synth.make_reads("c2", 4, seed=41)]
    text, offs, lens = _text(reads)
    t = torch.from_numpy(text).cuda()
    n = len(lens)

    def call(ptr, nbytes, kind, o=offs):
        return lib.mtr_upload_batch_device(eng.h, C.c_void_p(ptr), nbytes, o.ctypes.data, lens.ctypes.data, n, kind, None)

    def err():
        return lib.mtr_last_error(eng.h).decode()

    assert call(text.ctypes.data, len(text), mtr_amd.TEXT_ASCII) == 2 and "not device memory" in err()
    pinned = torch.from_numpy(text).pin_memory()
    assert call(pinned.data_ptr(), len(text), mtr_amd.TEXT_ASCII) == 2 and "not device memory" in err()
    assert call(t.data_ptr(), len(text), 7) == 2 and "text_kind" in err()
    assert call(t.data_ptr(), len(text) - 1, mtr_amd.TEXT_ASCII) == 2 and "outside the text" in err()
    assert call(0, len(text), mtr_amd.TEXT_ASCII) == 2
    assert call(t.data_ptr(), 0, mtr_amd.TEXT_ASCII) == 2
    assert eng.lib.mtr_run_resident(eng.h) == 2
    assert call(t.data_ptr(), len(text), mtr_amd.TEXT_ASCII) == 0
    eng.n_reads = n
    eng.run()
    assert eng.fetch() == _host(eng, reads)[0]


# ---- round trip on the device ---------------------------------------------------------------------------------------------
def test_export_tensor_equals_fetch_packed(eng):
    reads = [c for _, c in synth.make_reads("headline2k", 500, seed=51)]
    text, offs, lens = _text(reads, junk=True, seed=52)
    eng.process_device(torch.from_numpy(text).cuda(), offs, lens)
    blob, counts = eng.export_tensor()
    assert blob.device.type == "cuda" and blob.dtype == torch.uint8
    assert counts.device.type == "cpu" and counts.dtype == torch.int32
    want, wcnt = eng.fetch_packed()
    assert bytes(blob.cpu().numpy()) == want and len(want) > 0
    assert np.array_equal(counts.numpy(), wcnt)


def _alignments(e):
    """mtr_alignments for every record of the resident batch: (ops, offsets, ends)"""
    recs = C.POINTER(mtr_amd.CRecord)()
    cnts = C.POINTER(C.c_int32)()
    total = C.c_int64()
    e._check(e.lib.mtr_fetch_results(e.h, C.byref(recs), C.byref(cnts), C.byref(total)), "mtr_fetch_results")
    try:
        n = int(total.value)
        idx = np.repeat(np.arange(e.n_reads, dtype=np.int32), [cnts[i] for i in range(e.n_reads)])
        ops, off, end = C.POINTER(C.c_uint8)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
        e._check(e.lib.mtr_alignments(e.h, n, idx.ctypes.data_as(C.POINTER(C.c_int32)), recs, C.byref(ops), C.byref(off), C.byref(end)),
                 "mtr_alignments")
        o = np.ctypeslib.as_array(off, shape=(n + 1,)).copy()
        out = (bytes(np.ctypeslib.as_array(ops, shape=(max(int(o[-1]), 1),))[:int(o[-1])]), o, np.ctypeslib.as_array(end, shape=(max(2 * n, 1),))[:2 * n].copy())
        for p in (ops, off, end):
            mtr_amd._libc.free(C.cast(p, C.c_void_p))
        return n, out
    finally:
        e.lib.mtr_free_results(recs, cnts)


def test_alignments_after_a_device_upload(eng):
    reads = [c for _, c in synth.make_reads("c2", 200, seed=61)]
    eng.upload(reads)
    eng.run()
    n_host, want = _alignments(eng)
    text, offs, lens = _text(reads, lower=0.5, junk=True, seed=62)
    eng.upload_device(torch.from_numpy(text).cuda(), offs, lens)
    eng.run()
    n_dev, got = _alignments(eng)
    assert n_host == n_dev > 0
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
