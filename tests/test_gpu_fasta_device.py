"""A FASTA file's bytes in device memory on the MI355X: Engine.parse_fasta_device / upload_fasta_device (mtr_parse_fasta_device,
mtr_upload_fasta_device, the kernels of mtr_amd/csrc/fasta.hip.inc) against the reference reader's loop as tests/test_host_driver.py
restates it - on its hostile files, on files that put every special byte on the kernels' tile edges, on the three stop events - and
end to end against the reference's recorded stdout: file bytes in, mTR's stdout bytes out."""
import ctypes as C
import os

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu
from tests.test_host_driver import FASTA_CASES, reference_reader

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

T = mtr_amd.FASTA_TILE_BYTES
WINDOW = 4095
LUT = np.full(256, 255, np.uint8)
for _c, _v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
    LUT[_c] = _v


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


def rules(data: bytes):
    """reference_reader (handle_one_file.c:201-269) a window at a time, with the position of the stop:
    ([(id, codes)], end, bad_char, end_pos); end_pos = len(data) when the file ended"""
    reads, cur, n_cur, cur_id, have_header, pos = [], [], 0, b"", False, 0

    def close():
        reads.append((cur_id, np.concatenate(cur) if cur else np.zeros(0, np.uint8)))

    while pos < len(data):
        w = data[pos:pos + WINDOW]
        nl = w.find(b"\n")
        if nl >= 0:
            w = w[:nl + 1]
        start, pos = pos, pos + len(w)
        cut = len(w)
        for stop in (b"\0", b"\n", b"\r"):
            k = w.find(stop, 0, cut)
            if k >= 0:
                cut = k
        if w[:1] == b">":
            ident = w[1:cut]
            if not have_header:
                have_header, cur_id = True, ident
                continue
            if n_cur == 0:
                return reads, "empty", None, start
            close()
            cur, n_cur, cur_id = [], 0, ident
            continue
        codes = LUT[np.frombuffer(w[:cut], np.uint8)]
        bad = np.flatnonzero(codes == 255)
        good = int(bad[0]) if len(bad) else len(codes)
        if n_cur + good >= 1000000:
            return reads, "toolong", None, start + (1000000 - n_cur - 1)
        if len(bad):
            return reads, "bad", w[good:good + 1], start + good
        cur.append(codes)
        n_cur += len(codes)
    if n_cur:
        close()
        return reads, "eof", None, len(data)
    return reads, "empty", None, len(data)


def _device(data: bytes):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")


def _check(eng, data: bytes, buf=None, want=None):
    """parse_fasta_device on data (buf: the tensor that holds it) against the rules; returns the Fasta"""
    reads, end, bad_char, end_pos = want if want is not None else rules(data)
    f = eng.parse_fasta_device(_device(data) if buf is None else buf)
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


# ---- 1: the reference loop's own hostile files ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(FASTA_CASES))
def test_parse_equals_the_reference_loop(eng, case):
    data = FASTA_CASES[case]
    want = rules(data)
    ref_reads, ref_end = reference_reader(data)                   # rules() adds the stop's position to reference_reader and nothing else
    assert [(i, c.tolist()) for i, c in want[0]] == ref_reads
    assert ref_end == (want[1] if want[1] != "bad" else "bad:" + want[2].decode("latin1"))
    _check(eng, data, want=want)


# ---- 2: the kernels' own boundaries --------------------------------------------------------------------------------------------
def _seq(rng, n, lower=0.3):
    b = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, size=n)].copy()
    b[rng.rand(n) < lower] += 32
    return b.tobytes()


def _wrapped(rng, n, width, eol=b"\n"):
    s = _seq(rng, n)
    return eol.join(s[i:i + width] for i in range(0, n, width)) + eol


def _fill(rng, nbytes, width=60):
    """exactly nbytes of sequence lines wrapped at width; the last byte is a base"""
    out = _wrapped(rng, nbytes, width)[:nbytes]
    return out[:-1] + b"A" if out.endswith(b"\n") else out


def _tail(rng, have):
    """records behind the special byte, up to three tiles and a bit"""
    return b">tail one\n" + _wrapped(rng, max(3 * T + 50 - have, 100), 60) + b">tail two\n" + _wrapped(rng, 77, 60)


def _edge_files():
    rng = np.random.RandomState(5)
    out = {}
    for p in (T - 1, T, T + 1):
        head = b">a\n" + _fill(rng, p - 3)                         # p bytes: byte p is the next one
        out[f"lf_at_{p}"] = head + b"\n" + _wrapped(rng, 500, 60)
        out[f"header_at_{p}"] = head[:-1] + b"\n" + b">b at the edge\n" + _wrapped(rng, 500, 60)
        out[f"cr_at_{p}"] = head + b"\rNNNN hidden\n" + _wrapped(rng, 500, 60)
        out[f"nul_at_{p}"] = head + b"\0NNNN hidden\n" + _wrapped(rng, 500, 60)
        out[f"nul_in_header_at_{p}"] = head[:-12] + b"\n>id of b" + b"\0" + b"hidden\n" + _wrapped(rng, 500, 60)
        out[f"last_base_at_{p}"] = head + b"G\n>b\n" + _wrapped(rng, 500, 60)
        out[f"last_byte_of_file_at_{p}"] = head + b"G"
        # one long line whose second fgets window starts on byte p: a base there, and a '>' there (a header window in mid-line)
        ls = p - WINDOW
        pre = {0: b"", 1: b"\n", 2: b"A\n"}.get(ls) if ls < 3 else b">w\n" + _fill(rng, ls - 4) + b"\n"
        assert len(pre) == ls
        out[f"window_edge_at_{p}"] = pre + _seq(rng, WINDOW + 1500) + b"\n"
        out[f"gt_on_window_edge_at_{p}"] = pre + _seq(rng, WINDOW) + b">x\n" + _wrapped(rng, 300, 60)
        out[f"cr_before_window_edge_at_{p}"] = pre + _seq(rng, WINDOW - 1) + b"\r" + _seq(rng, 200) + b"\n"      # the CR hides nothing of the next window
    for k in list(out):
        if not k.startswith("last_byte_of_file"):
            out[k] += _tail(rng, len(out[k]))
            assert len(out[k]) >= 3 * T
    out["one_line_of_two_tiles"] = b">a\n" + _seq(rng, 2 * T + 17) + b"\n>b\nACGT\n"
    out["long_header_over_a_tile_edge"] = b">a\n" + _fill(rng, T - 2000) + b"\n>" + b"ACGT" * 1250 + b"\nACGT\n>c\n" + _wrapped(rng, 2 * T, 60)
    for width in (1, 15, 16, 17, 60):
        out[f"wrapped_{width}"] = b"".join(b">w%d_%d x\n" % (width, r) + _wrapped(rng, int(rng.randint(1, 3000)), width) for r in range(8))
    out["crlf"] = b"".join(b">r%d y\r\n" % r + _wrapped(rng, int(rng.randint(1, 3000)), 60, b"\r\n") for r in range(8))
    out["bad_in_a_later_tile"] = b">a\n" + _wrapped(rng, 2 * T, 60) + b">b\n" + _wrapped(rng, 100, 60) + b"ACGNT\n>c\nAC\n"
    out["empty_record_in_a_later_tile"] = b">a\n" + _wrapped(rng, 2 * T, 60) + b">b\n>c\n" + _wrapped(rng, T, 60)
    out["bad_in_an_empty_record"] = b">a\nACGT\n>b\nN\n>c\nAC\n"
    out["bad_after_an_empty_record"] = b">a\nACGT\n>b\n>c\nANC\n"
    out["header_only"] = b">only"
    return out


EDGE_FILES = _edge_files()


@pytest.mark.parametrize("name", sorted(EDGE_FILES))
def test_special_bytes_on_the_tile_edges(eng, name):
    f = _check(eng, EDGE_FILES[name])
    if name.startswith(("lf_at", "header_at", "last_base_at", "window_edge", "one_line", "long_header", "wrapped", "crlf")):
        assert f.end == "eof" and len(f.ids) >= 2


@pytest.mark.parametrize("at", [1, 2, 3])
@pytest.mark.parametrize("rest", [1, 2, 3])
def test_a_slice_at_an_unaligned_start(eng, at, rest):
    """the file is a slice of a larger tensor of 'N's: a byte taken from outside the slice would be a bad character"""
    rng = np.random.RandomState(10 * at + rest)
    data = b">s one\n" + _wrapped(rng, T + 300, 60) + b">s two\n" + _wrapped(rng, 900, 17)
    data += b"A" * ((rest - len(data)) % 4)
    assert len(data) % 4 == rest and len(data) > T
    big = torch.full((len(data) + 64,), ord("N"), dtype=torch.uint8, device="cuda")
    big[at:at + len(data)] = _device(data)
    buf = big[at:at + len(data)]
    assert buf.data_ptr() % 4 == at
    f = _check(eng, data, buf=buf)
    assert f.end == "eof" and len(f.ids) == 2


def test_more_tiles_than_one_step_of_the_tile_scan(eng):
    """the scans over the tiles take 1024 tiles a step: a file of more tiles, lines of A only, records that run over many tiles"""
    line = b"A" * 60 + b"\n"
    recs, n = [], 0
    while n < 1100 * T:
        recs.append(b">r%d\n" % len(recs) + line * (1 + 997 * (len(recs) % 3)))
        n += len(recs[-1])
    f = _check(eng, b"".join(recs))
    assert f.end == "eof" and len(f.ids) == len(recs)


# ---- 3: the stop events ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [0, 60])
def test_a_record_that_reaches_the_readers_limit(eng, width):
    rng = np.random.RandomState(3)
    huge = _seq(rng, 1000010)
    body = huge + b"\n" if width == 0 else b"\n".join(huge[i:i + width] for i in range(0, len(huge), width)) + b"\n"
    data = b">ok\nACGT\n>ok too\nGGCCA\n>huge\n" + body + b">good\nACGT\n"
    want = rules(data)
    assert want[1] == "toolong" and [i for i, _ in want[0]] == [b"ok", b"ok too"]
    _check(eng, data, want=want)


def test_a_record_one_base_beyond_the_longest_read(eng):
    rng = np.random.RandomState(4)
    data = b">long\n" + _wrapped(rng, mtr_amd.MAX_READ_LENGTH + 1, 60)
    buf = _device(data)
    f = _check(eng, data, buf=buf)
    assert f.end == "eof" and f.lens.tolist() == [mtr_amd.MAX_READ_LENGTH + 1]
    with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: read 0: length 833334"):
        eng.upload_fasta_device(buf)
    with pytest.raises(mtr_amd.MtrError, match="no batch uploaded"):
        eng.run()
    good = eng.upload_fasta_device(_device(b">t\n" + b"TTAGGG" * 80 + b"\n"))
    eng.run()
    assert good.ids == [b"t"] and len(eng.fetch()[0]) >= 1


def test_reads_before_a_bad_character_are_uploaded(eng):
    src = open(gu.input_path("synth_c2")).read().split(">")[1:]
    data = ("".join(">" + r for r in src[:5]) + ">bad\nACGTNACGT\n>never\nACGT\n").encode()
    f = eng.upload_fasta_device(_device(data))
    assert (f.end, f.bad_char, f.text) == ("bad", b"N", None) and f.end_pos == data.index(b"NACGT")
    assert f.ids == [r.split("\n", 1)[0].encode() for r in src[:5]] and eng.n_reads == 5
    eng.run()
    got, blob = eng.fetch(), eng.fetch_packed()
    reads = [c for _, c in gu.read_fasta(gu.input_path("synth_c2"))][:5]
    assert f.lens.tolist() == [len(r) for r in reads]
    eng.upload(reads)
    eng.run()
    assert got == eng.fetch() and blob[0] == eng.fetch_packed()[0] and sum(len(g) for g in got) > 0


@pytest.mark.parametrize("data", [b"", b">only a header\n"], ids=["empty", "header_only"])
def test_no_reads_is_no_batch(eng, data):
    eng.upload([np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 40)])          # a batch that the call below must not leave behind
    f = eng.upload_fasta_device(_device(data))
    assert (f.ids, f.end, f.bad_char, f.end_pos, len(f.lens)) == ([], "empty", None, len(data), 0)
    with pytest.raises(mtr_amd.MtrError, match="no batch uploaded"):
        eng.run()
    p = eng.parse_fasta_device(_device(data))
    assert (p.ids, p.end, p.end_pos, p.text.numel()) == ([], "empty", len(data), 0)


# ---- 4: file bytes in, the reference's stdout bytes out ---------------------------------------------------------------------------
def _golden(name, mode):
    p = os.path.join(gu.GOLDEN, f"{name}.{mode}.stdout")
    return open(p, "rb").read() if os.path.exists(p) else None


@pytest.mark.parametrize("name", ["3_5", "edge", "synth_c2", "synth_c3"])
def test_file_bytes_in_stdout_bytes_out(eng, eng_p, name):
    raw = open(gu.input_path(name), "rb").read()
    buf = _device(raw)
    f = eng.upload_fasta_device(buf)
    assert f.end == "eof" and f.end_pos == len(raw)
    eng.run()
    assert eng.report_bytes(f.ids) == _golden(name, "default")
    if _golden(name, "a") is not None:
        assert eng.report_bytes(f.ids, alignments=True) == _golden(name, "a")
    if name in ("edge", "synth_c2"):
        fp = eng_p.upload_fasta_device(buf)
        eng_p.run()
        assert eng_p.report_bytes(fp.ids) == _golden(name, "p")


def test_headline_shaped_batch_equals_the_host_upload(eng):
    named = synth.make_reads("headline2k", 500, seed=71)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parts = []
    for rid, codes in named:
        s = acgt[codes].tobytes()
        parts.append(b">" + str(rid).encode() + b"\n" + b"\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + b"\n")
    f = eng.upload_fasta_device(_device(b"".join(parts)))
    assert f.end == "eof" and f.ids == [str(rid).encode() for rid, _ in named] and f.lens.tolist() == [len(c) for _, c in named]
    eng.run()
    got = eng.fetch_packed()
    eng.upload([c for _, c in named])
    eng.run()
    want = eng.fetch_packed()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and len(want[0]) > 0


# ---- 5: stream order -------------------------------------------------------------------------------------------------------------
def test_file_written_by_torch_just_before_the_call(eng):
    """the buffer is filled by a copy on a side stream behind a few ms of other work there, with no synchronise: the kernels must wait
    for it (an event on that stream); before the copy the buffer holds only 'N's"""
    rng = np.random.RandomState(8)
    data = b"".join(b">s%d\n" % r + _wrapped(rng, 2000, 60) for r in range(200))
    want = rules(data)
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


# ---- 6: refusals through the C-ABI -----------------------------------------------------------------------------------------------
def test_library_refuses_bad_buffers_and_small_destinations(eng):
    lib = eng.lib
    rng = np.random.RandomState(9)
    data = b"".join(b">q%d some id\n" % r + _wrapped(rng, 700, 60) for r in range(6))
    host = np.frombuffer(data, np.uint8).copy()
    t = torch.from_numpy(host).cuda()
    info = mtr_amd.CFastaInfo()

    def parse(ptr, nbytes, dst=None):
        return lib.mtr_parse_fasta_device(eng.h, C.c_void_p(ptr), nbytes, None, dst, C.byref(info))

    def err():
        return lib.mtr_last_error(eng.h).decode()

    assert parse(host.ctypes.data, len(data)) == 2 and "not device memory" in err()
    pinned = torch.from_numpy(host).pin_memory()
    assert parse(pinned.data_ptr(), len(data)) == 2 and "not device memory" in err()
    assert parse(0, len(data)) == 2 and "NULL" in err()
    assert parse(t.data_ptr(), -1) == 2 and "n_bytes -1" in err()
    assert parse(t.data_ptr(), 1 << 31) == 2 and "n_bytes" in err()
    assert parse(t.data_ptr(), t.untyped_storage().nbytes() + (64 << 20)) == 2 and "runs past the end" in err()
    for fn in (lambda: lib.mtr_upload_fasta_device(eng.h, C.c_void_p(host.ctypes.data), len(data), None, C.byref(info)),
               lambda: lib.mtr_upload_fasta_device(eng.h, None, len(data), None, C.byref(info))):
        assert fn() == 2
    # sizes only, then every capacity one below them: MTR_ERR_OVERFLOW, the sizes filled in, not a byte written
    assert parse(t.data_ptr(), len(data)) == 0
    n, nb, ni = info.n_reads, info.n_bases, info.id_bytes
    assert (n, nb, ni, info.end) == (6, 6 * 700, sum(len(b"q%d some id" % r) for r in range(6)), 0)
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
    _check(eng, data, buf=t)                                      # the engine is usable afterwards


# ---- 7: the largest file the entry points take --------------------------------------------------------------------------------------
def test_a_file_of_int32_max_bytes(eng):
    """positions and base counts beyond 2^30 and up to 2^31 - 1: 2^25 records of 61 bases, made and checked on the device through the
    C-ABI (a Python list of 33 million IDs is not what is tested); then a bad character ten bytes before the end"""
    n, n_rec = (1 << 31) - 1, 1 << 25
    buf = torch.from_numpy(np.frombuffer(b">\n" + b"A" * 61 + b"\n", np.uint8).copy()).cuda().repeat(n_rec)[:n]
    info = mtr_amd.CFastaInfo()

    def parse(dst=None):
        eng._check(eng.lib.mtr_parse_fasta_device(eng.h, C.c_void_p(buf.data_ptr()), n, None, dst, C.byref(info)), "mtr_parse_fasta_device")
        return info.n_reads, info.end, info.end_pos, info.n_bases, info.id_bytes

    torch.cuda.synchronize()
    assert parse() == (n_rec, 0, n, 61 * n_rec, 0)
    text = torch.zeros(61 * n_rec, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(n_rec, dtype=torch.int64, device="cuda")
    lens = torch.zeros(n_rec, dtype=torch.int32, device="cuda")
    id_off = torch.ones(n_rec + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dst = mtr_amd.CFastaDst(text.data_ptr(), offsets.data_ptr(), lens.data_ptr(), None, id_off.data_ptr(), text.numel(), n_rec, 0)
    assert parse(C.byref(dst)) == (n_rec, 0, n, 61 * n_rec, 0)
    assert bool((text == ord("A")).all()) and bool((lens == 61).all()) and bool((id_off == 0).all())
    assert torch.equal(offsets, torch.arange(n_rec, dtype=torch.int64, device="cuda") * 61)
    del text, offsets, lens, id_off
    buf[n - 10] = ord("N")
    torch.cuda.synchronize()
    assert parse() == (n_rec - 1, 2, n - 10, 61 * (n_rec - 1), 0) and info.bad_char == ord("N")
