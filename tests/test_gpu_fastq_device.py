"""A FASTQ file's bytes in device memory on the MI355X: Engine.parse_fastq_device / upload_fastq_device (mtr_parse_fastq_device,
mtr_upload_fastq_device(_in_file), the kernels of mtr_amd/csrc/fastq.hip.inc) against fastq_rules of tests/test_fastq_device.py, the
rules of include/mtr_hip.h restated in Python - on hand-written files with every stop, on files that put every special byte on the
kernels' tile and span edges, on random files - and end to end: the goldens' records written as FASTQ give the reference's stdout."""
import ctypes as C
import os

import numpy as np
import pytest

import mtr_amd
from tests import golden_util as gu
from tests.test_fastq_device import LUT, fastq_rules, random_records, to_fasta, to_fastq
from tests.test_host_driver import reference_reader

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

T = mtr_amd.FASTA_TILE_BYTES
ACGT = np.frombuffer(b"ACGT", np.uint8).copy()


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


def _device(data: bytes):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")


def _check(eng, data: bytes, buf=None, want=None):
    """parse_fastq_device on data (buf: the tensor that holds it) against the rules; returns the Fasta"""
    reads, end, bad_char, end_pos = want if want is not None else fastq_rules(data)
    f = eng.parse_fastq_device(_device(data) if buf is None else buf)
    assert (f.end, f.bad_char, f.end_pos) == (end, bad_char, end_pos)
    assert f.ids == [i for i, _ in reads]
    assert f.lens.dtype == np.int32 and f.offsets.dtype == np.int64
    assert f.lens.tolist() == [len(c) for _, c in reads]
    assert f.offsets.tolist() == (np.cumsum(f.lens, dtype=np.int64) - f.lens).tolist()          # the exclusive sum
    text = f.text.cpu().numpy()
    assert f.text.device.type == "cuda" and f.text.dtype == torch.uint8 and len(text) == int(f.lens.sum())
    codes = LUT[text]                                                                           # only ACGTacgt, the file's own bytes
    assert (codes < 4).all()
    want_codes = np.concatenate([c for _, c in reads]) if reads else np.zeros(0, np.uint8)
    assert np.array_equal(codes, want_codes)
    return f


# ---- 1: files written by hand ----------------------------------------------------------------------------------------------------
# A file is a list of records, a record its four lines without their ends: [header, sequence, separator, quality].
def _good():
    return [[b"@r0", b"ACGTACGT", b"+", b"IIIIIIII"], [b"@r1 with words", b"GGCC", b"+", b"!!!!"], [b"@r2", b"TTAGGGTTAGGG", b"+", b"FFFFFFFFFFFF"],
            [b"@r3", b"CA", b"+", b"II"]]


def _join(recs, eol=b"\n", last_eol=True):
    out = b"".join(line + eol for rec in recs for line in rec)
    return out if last_eol or not out else out[:len(out) - len(eol)]


def _set(line, value):
    def change(rec):
        rec[line] = value(rec[line]) if callable(value) else value
    return change


def _empty_sequence(rec):
    rec[1], rec[3] = b"", b""


# kind -> (what it does to one record, the end it gives)
CHANGES = {
    "lower_case": (_set(1, bytes.lower), "eof"),
    "empty_id": (_set(0, b"@"), "eof"),
    "nul_in_header": (_set(0, b"@ab\0cd"), "eof"),
    "cr_in_header": (_set(0, b"@ab\rcd"), "eof"),
    "nul_in_quality": (_set(3, lambda q: q[:1] + b"\0" + q[2:]), "format"),
    "cr_in_quality": (_set(3, lambda q: q[:1] + b"\r" + q[2:]), "format"),
    "quality_begins_with_at": (_set(3, lambda q: b"@" + q[1:]), "eof"),
    "quality_begins_with_gt": (_set(3, lambda q: b">" + q[1:]), "eof"),
    "quality_begins_with_plus": (_set(3, lambda q: b"+" + q[1:]), "eof"),
    "separator_repeats_id": (lambda rec: rec.__setitem__(2, b"+" + rec[0][1:]), "eof"),
    "stop_n": (_set(1, lambda s: s[:1] + b"N" + s[2:]), "bad"),
    "stop_empty_sequence": (_empty_sequence, "empty"),
    "stop_header_without_at": (_set(0, lambda h: b">" + h[1:]), "format"),
    "stop_separator_without_plus": (_set(2, b"-"), "format"),
    "stop_quality_shorter": (_set(3, lambda q: q[:-1]), "format"),
    "stop_quality_longer": (_set(3, lambda q: q + b"I"), "format"),
}


def _hand_files():
    files = {}
    for eol, e in ((b"\n", "lf"), (b"\r\n", "crlf")):
        for last in (True, False):
            files[f"{e}_last_line_{'with' if last else 'without'}_end"] = (_join(_good(), eol, last), "eof", 4)
    for kind, (change, end) in CHANGES.items():
        for k in (0, 2):
            recs = _good()
            change(recs[k])
            files[f"{kind}_in_record_{k}"] = (_join(recs), end, 4 if end == "eof" else k)
    for k in (0, 2):
        for lines in (1, 2, 3):
            files[f"stop_cut_after_{lines}_lines_of_record_{k}"] = (_join(_good()[:k]) + _join([_good()[k][:lines]]), "format", k)
        files[f"stop_cut_inside_line_2_of_record_{k}"] = (_join(_good()[:k]) + _join([_good()[k][:2]], last_eol=False), "format", k)
        files[f"stop_trailing_blank_line_behind_record_{k}"] = (_join(_good()[:k + 1]) + b"\n", "format", k + 1)
    return files


HAND_FILES = _hand_files()


@pytest.mark.parametrize("name", sorted(HAND_FILES))
def test_files_written_by_hand(eng, name):
    data, end, n_reads = HAND_FILES[name]
    f = _check(eng, data)
    assert (f.end, len(f.ids)) == (end, n_reads)
    if "cut" in name:
        assert f.end_pos == len(data)
    if "trailing_blank" in name:
        assert f.end_pos == len(data) - 1


# ---- 2: the kernels' own boundaries: tiles of T bytes, spans of 16 ------------------------------------------------------------------
def _filler(size):
    """one good record of exactly `size` bytes (size >= 8)"""
    ident = b"" if size % 2 == 0 else b"x"
    k = (size - 6 - len(ident)) // 2
    assert k >= 1
    rec = b"@" + ident + b"\n" + b"ACGT" * (k // 4) + b"ACGT"[:k % 4] + b"\n+\n" + b"I" * k + b"\n"
    assert len(rec) == size
    return rec


# the target record ends its lines with CR LF; where its special bytes are, by its ID's and its sequence's lengths
OFFSETS = {"at": lambda i, m: 0, "cr": lambda i, m: 1 + i, "lf": lambda i, m: 2 + i, "first_base": lambda i, m: 3 + i,
           "last_base": lambda i, m: 2 + i + m, "plus": lambda i, m: 5 + i + m, "first_quality": lambda i, m: 8 + i + m}


def _placed(kind, pos, quality_first=b"I"):
    """a file whose second (or first) record has its byte `kind` at `pos`"""
    for i in range(9):
        for m in range(1, 5):
            room = pos - OFFSETS[kind](i, m)
            if room == 0 or room >= 8:
                target = b"@" + b"idididid"[:i] + b"\r\n" + b"gatc"[:m] + b"\r\n+\r\n" + quality_first + b"I" * (m - 1) + b"\r\n"
                data = (_filler(room) if room else b"") + target + _filler(23) + _filler(8)
                at = room + OFFSETS[kind](i, m)
                assert at == pos and data[at:at + 1] == {"at": b"@", "cr": b"\r", "lf": b"\n", "first_base": b"g", "last_base": b"gatc"[m - 1:m], "plus": b"+",
                                                          "first_quality": quality_first}[kind]
                return data, 4 if room else 3
    raise AssertionError((kind, pos))


@pytest.mark.parametrize("pos", [15, 16, 17, T - 1, T, T + 1])
@pytest.mark.parametrize("kind", sorted(OFFSETS))
def test_special_bytes_on_the_tile_and_span_edges(eng, kind, pos):
    data, n_reads = _placed(kind, pos)
    f = _check(eng, data)
    assert (f.end, len(f.ids)) == ("eof", n_reads)


def test_a_sequence_line_over_three_tiles(eng):
    rng = np.random.RandomState(21)
    recs = [(b"before", b"ACGTA" * 20)] + random_records(rng, 1, 2 * T + 5, 2 * T + 5) + [(b"behind", b"ttagg")]
    data = to_fastq(recs)
    start = data.index(recs[1][1])
    assert start // T + 2 == (start + 2 * T + 4) // T                  # its first and last base are two tile edges apart
    f = _check(eng, data)
    assert f.end == "eof" and f.lens.tolist() == [100, 2 * T + 5, 5]


def test_a_quality_line_that_begins_with_at_on_a_tile_edge(eng):
    data, n_reads = _placed("first_quality", T, quality_first=b"@")
    assert data[T - 1:T + 1] == b"\n@"
    f = _check(eng, data)
    assert (f.end, len(f.ids)) == ("eof", n_reads)


@pytest.mark.parametrize("tile_end", [T, 2 * T])
def test_a_bad_character_as_the_last_byte_of_a_tile(eng, tile_end):
    head = _filler(tile_end - 1 - 8) + b"@n\nACGTA"                     # the next byte is byte tile_end - 1
    data = head + b"N" + b"ACGT\n+\n" + b"I" * 10 + b"\n" + _filler(30)
    assert len(head) == tile_end - 1
    f = _check(eng, data)
    assert (f.end, f.bad_char, f.end_pos, len(f.ids)) == ("bad", b"N", tile_end - 1, 1)


@pytest.mark.parametrize("at", [1, 2, 3])
@pytest.mark.parametrize("rest", [1, 2, 3])
def test_a_slice_at_an_unaligned_start(eng, at, rest):
    """the file is a slice of a larger tensor of 'N's, its length 1 .. 3 beyond a multiple of 16: the unaligned dword path and the
    bytewise tail; a byte taken from outside the slice would show"""
    rng = np.random.RandomState(10 * at + rest)
    data = to_fastq(random_records(rng, 40, 50, 300))
    data += _filler(8 + (rest - len(data) - 8) % 16)
    assert len(data) % 16 == rest and len(data) > T
    big = torch.full((len(data) + 64,), ord("N"), dtype=torch.uint8, device="cuda")
    big[at:at + len(data)] = _device(data)
    buf = big[at:]
    assert buf.data_ptr() % 4 == at
    _check(eng, data + b"N" * (64 - at), buf=buf)                      # the whole rest of the tensor: the file, then a header line without '@'
    buf = big[at:at + len(data)]
    f = _check(eng, data, buf=buf)
    assert f.end == "eof" and len(f.ids) == 41
    up = eng.upload_fastq_device(buf)                                  # the packing kernel reads the reads out of the slice itself
    assert up.lens.tolist() == f.lens.tolist() and up.ids == f.ids


def test_more_tiles_than_one_step_of_the_tile_scan(eng):
    """1025 tiles and 7 bytes of short records: the one-workgroup scans take 1024 tiles a step, the record scans 1024 records"""
    rng = np.random.RandomState(22)
    n, parts, have = 1025 * T + 7, [], 0
    lens = rng.randint(20, 41, size=n // 46)
    for k, m in enumerate(lens.tolist()):
        rec = b"@%x\n" % k + ACGT[rng.randint(0, 4, m)].tobytes() + b"\n+\n" + b"5" * m + b"\n"
        if have + len(rec) + 100 > n:
            break
        parts.append(rec)
        have += len(rec)
    parts.append(_filler(n - have))
    data = b"".join(parts)
    assert len(data) == n
    f = _check(eng, data)
    assert f.end == "eof" and len(f.ids) == len(parts) > 50000


# ---- 3: the limits ---------------------------------------------------------------------------------------------------------------
def _long_record(n_bases):
    """on the device: a good record, then one whose sequence line has n_bases bases, then a good one"""
    head, tail = _device(b"@ok\nACGT\n+\nIIII\n@long\n"), _device(_filler(20))
    seq = torch.from_numpy(ACGT).cuda()[torch.arange(n_bases, device="cuda") % 4]
    return torch.cat([head, seq, _device(b"\n+\n"), torch.full((n_bases,), ord("I"), dtype=torch.uint8, device="cuda"), _device(b"\n"), tail]), head.numel()


def test_a_sequence_line_that_reaches_the_readers_limit(eng):
    buf, start = _long_record(1000000)
    f = eng.parse_fastq_device(buf)
    assert (f.end, f.bad_char, f.end_pos, f.ids, f.lens.tolist()) == ("toolong", None, start + 999999, [b"ok"], [4])
    buf, start = _long_record(999999)                                  # one base fewer: no stop
    f = eng.parse_fastq_device(buf)
    assert (f.end, f.end_pos, f.lens.tolist()) == ("eof", buf.numel(), [4, 999999, 7])


def test_a_record_one_base_beyond_the_longest_read(eng):
    buf, _ = _long_record(mtr_amd.MAX_READ_LENGTH + 1)
    data = buf.cpu().numpy().tobytes()
    f = _check(eng, data, buf=buf)
    assert f.end == "eof" and f.lens.tolist() == [4, mtr_amd.MAX_READ_LENGTH + 1, 7]
    with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: read 1: length 833334"):
        eng.upload_fastq_device(buf)
    with pytest.raises(mtr_amd.MtrError, match="no batch uploaded"):
        eng.run()
    good = eng.upload_fastq_device(_device(to_fastq([(b"t", b"TTAGGG" * 80)])))
    eng.run()
    assert good.ids == [b"t"] and len(eng.fetch()[0]) >= 1


@pytest.mark.parametrize("data", [b"", b"@only a header\n"], ids=["empty", "header_only"])
def test_no_reads_is_no_batch(eng, data):
    eng.upload([np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 40)])          # a batch that the call below must not leave behind
    f = eng.upload_fastq_device(_device(data))
    assert (f.ids, f.end, f.bad_char, f.end_pos, len(f.lens)) == ([], "format" if data else "empty", None, len(data), 0)
    with pytest.raises(mtr_amd.MtrError, match="no batch uploaded"):
        eng.run()
    p = eng.parse_fastq_device(_device(data))
    assert (p.ids, p.end, p.end_pos, p.text.numel()) == ([], f.end, len(data), 0)


# ---- 4: random files ---------------------------------------------------------------------------------------------------------------
def _random_file(seed):
    rng = np.random.RandomState(1000 + seed)
    recs = [[b"@" + i, s, b"+" + (i if rng.rand() < 0.2 else b""), bytes(rng.randint(33, 127, len(s)).astype(np.uint8))] for i, s in random_records(rng, 200)]
    eol = b"\r\n" if rng.rand() < 0.3 else b"\n"
    if seed % 2 == 0:
        return _join(recs, eol, rng.rand() < 0.5), None
    k, kinds = int(rng.randint(0, 200)), sorted(k for k, (_, end) in CHANGES.items() if end != "eof") + ["cut", "blank"]
    kind = kinds[rng.randint(len(kinds))]
    if kind == "cut":
        return _join(recs[:k], eol) + _join([recs[k][:int(rng.randint(1, 4))]], eol, rng.rand() < 0.5), k
    if kind == "blank":
        return _join(recs, eol) + eol, 200
    if kind == "stop_n":
        at = int(rng.randint(len(recs[k][1])))
        recs[k][1] = recs[k][1][:at] + b"N" + recs[k][1][at + 1:]
    elif kind in ("nul_in_quality", "cr_in_quality") and len(recs[k][3]) == 1:
        recs[k][3] = b"\0"
    else:
        CHANGES[kind][0](recs[k])
    return _join(recs, eol), k


@pytest.mark.parametrize("seed", range(40))
def test_random_files(eng, seed):
    data, stopped_in = _random_file(seed)
    f = _check(eng, data)
    assert (f.end == "eof") == (stopped_in is None) and len(f.ids) == (200 if stopped_in is None else stopped_in)


# ---- 5: file bytes in, the reference's stdout bytes out ---------------------------------------------------------------------------
def _golden(name, mode):
    p = os.path.join(gu.GOLDEN, f"{name}.{mode}.stdout")
    return open(p, "rb").read() if os.path.exists(p) else None


@pytest.mark.parametrize("name", ["3_5", "edge", "synth_c2", "synth_c3"])
def test_golden_records_as_fastq_give_the_recorded_stdout(eng, eng_p, name):
    raw = open(gu.input_path(name), "rb").read()
    reads, end = reference_reader(raw)
    assert end == "eof"
    fastq = to_fastq([(i, ACGT[np.asarray(c, np.uint8)].tobytes()) for i, c in reads], repeat_id=True)
    buf, fasta = _device(fastq), _device(raw)
    f = eng.upload_fastq_device(buf)
    assert (f.end, f.end_pos, f.text) == ("eof", len(fastq), None) and f.ids == [i for i, _ in reads]
    eng.run()
    assert eng.report_bytes(f.ids) == _golden(name, "default")
    if _golden(name, "a") is not None:
        assert eng.report_bytes(f.ids, alignments=True) == _golden(name, "a")
    for e in (eng, eng_p):
        fq = e.upload_fastq_device(buf)
        e.run()
        got = e.fetch()
        fa = e.upload_fasta_device(fasta)
        e.run()
        assert got == e.fetch() and fq.ids == fa.ids and fq.lens.tolist() == fa.lens.tolist() and sum(len(g) for g in got) > 0


# ---- 6: file-order mode ------------------------------------------------------------------------------------------------------------
def test_two_chunks_through_a_file_state_equal_the_fasta_chunks(eng):
    """the FASTQ chunks through one state, with a refused chunk between them, against the FASTA chunks of the same records through another"""
    rng = np.random.RandomState(99)
    recs = [(b"f%d" % k, ACGT[rng.randint(0, 4, size=n)].tobytes()) for k, n in enumerate((5000, 700, 1500, 650, 600, 649))]
    too_long, _ = _long_record(mtr_amd.MAX_READ_LENGTH + 1)
    fsq, fsa = mtr_amd.FileState(), mtr_amd.FileState()
    for chunk, part in enumerate((recs[:2], recs[2:])):
        fa = eng.upload_fasta_device(_device(to_fasta(part)), file_state=fsa)
        want_tail = eng.test_file_tail()
        eng.run()
        want = eng.fetch()
        fq = eng.upload_fastq_device(_device(to_fastq(part)), file_state=fsq)
        tail = eng.test_file_tail()
        eng.run()
        assert fq.ids == fa.ids and fq.lens.tolist() == fa.lens.tolist() and eng.fetch() == want
        for k in range(3):
            assert tail[k].dtype == want_tail[k].dtype and np.array_equal(tail[k], want_tail[k]), k
        if chunk == 0:
            with pytest.raises(mtr_amd.MtrError, match="read 1: length 833334"):
                eng.upload_fastq_device(too_long, file_state=fsq)
    assert want_tail[0].any() and want_tail[2].any()                    # the second chunk found stale tails and after-bases
    fsq.close()
    fsa.close()


# ---- 7: stream order -------------------------------------------------------------------------------------------------------------
def test_file_written_by_torch_just_before_the_call(eng):
    """the buffer is filled by a copy on a side stream behind a few ms of other work there, with no synchronise: the kernels must wait
    for it (an event on that stream); before the copy the buffer holds only 'N's"""
    data = to_fastq(random_records(np.random.RandomState(8), 200, 1500, 2500))
    want = fastq_rules(data)
    dev = torch.device("cuda", 0)
    src = _device(data)
    buf = torch.full((len(data),), ord("N"), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        x = torch.randn(4096, 4096, device=dev)
        for _ in range(6):
            x = x @ x / 64.0                                      # (keeps the stream busy)
        buf.copy_(src, non_blocking=True)
        f = _check(eng, data, buf=buf, want=want)
    assert f.end == "eof" and len(f.ids) == 200
    torch.cuda.synchronize()


# ---- 8: refusals through the C-ABI -----------------------------------------------------------------------------------------------
def test_library_refuses_bad_buffers_and_small_destinations(eng):
    lib = eng.lib
    recs = [(b"q%d some id" % r, s) for r, (_, s) in enumerate(random_records(np.random.RandomState(9), 6, 700, 700))]
    data = to_fastq(recs)
    host = np.frombuffer(data, np.uint8).copy()
    t = torch.from_numpy(host).cuda()
    info = mtr_amd.CFastaInfo()

    def parse(ptr, nbytes, dst=None):
        return lib.mtr_parse_fastq_device(eng.h, C.c_void_p(ptr), nbytes, None, dst, C.byref(info))

    def err():
        return lib.mtr_last_error(eng.h).decode()

    assert parse(host.ctypes.data, len(data)) == 2 and "not device memory" in err()
    pinned = torch.from_numpy(host).pin_memory()
    assert parse(pinned.data_ptr(), len(data)) == 2 and "not device memory" in err()
    assert parse(0, len(data)) == 2 and "d_fastq is NULL" in err()
    assert parse(t.data_ptr(), -1) == 2 and "n_bytes -1" in err()
    assert parse(t.data_ptr(), 1 << 31) == 2 and "n_bytes" in err()
    assert parse(t.data_ptr(), t.untyped_storage().nbytes() + (64 << 20)) == 2 and "runs past the end" in err()
    fs = mtr_amd.FileState()
    for fn in (lambda: lib.mtr_upload_fastq_device(eng.h, C.c_void_p(host.ctypes.data), len(data), None, C.byref(info)),
               lambda: lib.mtr_upload_fastq_device(eng.h, None, len(data), None, C.byref(info)),
               lambda: lib.mtr_upload_fastq_device_in_file(eng.h, fs.h, C.c_void_p(host.ctypes.data), len(data), None, C.byref(info)),
               lambda: lib.mtr_upload_fastq_device_in_file(eng.h, None, C.c_void_p(t.data_ptr()), len(data), None, C.byref(info))):
        assert fn() == 2
    fs.close()
    # sizes only, then every capacity one below them: MTR_ERR_OVERFLOW, the sizes filled in, not a byte written
    assert parse(t.data_ptr(), len(data)) == 0
    n, nb, ni = info.n_reads, info.n_bases, info.id_bytes
    assert (n, nb, ni, info.end) == (6, 6 * 700, sum(len(i) for i, _ in recs), 0)
    cols = [torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((n,), -7, dtype=torch.int64, device="cuda"),
            torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((ni,), 0x5A, dtype=torch.uint8, device="cuda"),
            torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")]
    before = [c.clone() for c in cols]
    torch.cuda.synchronize()
    for caps in ((nb - 1, n, ni), (nb, n - 1, ni), (nb, n, ni - 1)):
        info = mtr_amd.CFastaInfo()
        dst = mtr_amd.CFastaDst(*[c.data_ptr() for c in cols], *caps)
        assert parse(t.data_ptr(), len(data), C.byref(dst)) == 5 and "needed" in err()
        assert (info.n_reads, info.n_bases, info.id_bytes) == (n, nb, ni)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(cols, before))
    dst = mtr_amd.CFastaDst(*[c.data_ptr() for c in cols], nb, n, ni)
    assert parse(t.data_ptr(), len(data), C.byref(dst)) == 0
    assert cols[2].tolist() == [700] * 6 and cols[4].tolist()[-1] == ni and cols[3].cpu().numpy().tobytes().startswith(b"q0 some idq1")
    # mtr_fasta_index answers after a FASTQ upload as after a FASTA one
    assert lib.mtr_upload_fastq_device(eng.h, C.c_void_p(t.data_ptr()), len(data), None, C.byref(info)) == 0 and info.n_reads == 6
    lens, id_off, ids = np.zeros(6, np.int32), np.zeros(7, np.int64), np.zeros(ni, np.uint8)
    assert lib.mtr_fasta_index(eng.h, lens.ctypes.data, id_off.ctypes.data, ids.ctypes.data) == 0
    assert lens.tolist() == [700] * 6 and id_off.tolist() == np.cumsum([0] + [len(i) for i, _ in recs]).tolist()
    assert ids.tobytes() == b"".join(i for i, _ in recs)
    _check(eng, data, buf=t)                                      # the engine is usable afterwards
