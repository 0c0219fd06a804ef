"""A FASTA or FASTQ file in device memory walked batch by batch on the MI355X: parse_*_device / upload_*_device with more=True
(mtr_parse_fasta_device_window, mtr_upload_fasta_device_window and their FASTQ twins) and Engine.walk_fasta_device /
walk_fastq_device.  The contract is WALK EQUIVALENCE: for a file and any window sizes, the reads concatenated over the walk (IDs,
lengths, base codes) are those of the whole file by rules() / fastq_rules(); the last item's end, bad_char and absolute end_pos are the
whole file's; every earlier item says "more".  Beyond that every single call is held against window_model
(tests/test_walk_device.py), the window rules of include/mtr_hip.h in Python, which includes that a window returns every read it
can.  The files and what is claimed about them here are checked on the model, without a GPU, in tests/test_walk_device.py."""
import ctypes as C
import os

import numpy as np
import pytest

import mtr_amd
from tests import golden_util as gu
from tests.test_fastq_device import fastq_rules, to_fastq
from tests.test_host_driver import FASTA_CASES
from tests.test_walk_device import (ACGT, FASTQ_STOPS, FO, HAND, WALK_WINDOWS, fourth_lfs, golden_fastq, golden_raw, header_windows, walk_model,
                                    whole, window_model)

torch = pytest.importorskip("torch")

from tests.test_gpu_fasta_device import LUT, rules  # noqa: E402
from tests.test_gpu_file_order_device import _capture, _rec  # noqa: E402

pytestmark = pytest.mark.gpu

T = mtr_amd.FASTA_TILE_BYTES
WINDOW = 4095
MAX_CALLS = 48            # per walk of a hostile file: a walk is its widenings (log2 of the longest record) and a call per batch


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _device(data: bytes):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")


def _parse(eng, fmt, buf, more):
    return (eng.parse_fasta_device if fmt == "fasta" else eng.parse_fastq_device)(buf, more=more)


def _item(f, pos=0):
    """a parsed Fasta as the model writes an item: ([(id, codes)], end, bad_char, absolute end_pos)"""
    text = LUT[f.text.cpu().numpy()]
    assert len(text) == int(f.lens.sum()) and f.offsets.tolist() == (np.cumsum(f.lens, dtype=np.int64) - f.lens).tolist()
    reads = [(i, text[int(o):int(o) + int(n)].tolist()) for i, o, n in zip(f.ids, f.offsets, f.lens)]
    return reads, f.end, f.bad_char, pos + f.end_pos


def _model_item(fmt, data, more, pos=0):
    reads, end, bad, end_pos = window_model(fmt, data, more)
    return [(i, np.asarray(c).tolist()) for i, c in reads], end, bad, pos + end_pos


def _assert_equivalent(fmt, data, items):
    reads, end, bad, pos = whole(fmt, data)
    assert [r for it in items for r in it[0]] == reads
    assert items[-1][1:] == (end, bad, pos)
    assert all(it[1] == "more" for it in items[:-1])


def _parse_walk(eng, fmt, data, buf, w, max_calls=None):
    """the walk of Engine.walk_*_device made of parse calls, so that the base codes come back; every call against the model"""
    items, pos, calls = [], 0, 0
    while True:
        k = min(w, len(data) - pos)
        more = pos + k < len(data)
        it = _item(_parse(eng, fmt, buf[pos:pos + k], more), pos)
        assert it == _model_item(fmt, data[pos:pos + k], more, pos), (pos, k, more)
        calls += 1
        assert max_calls is None or calls <= max_calls
        if it[1] == "more" and not it[0]:
            w *= 2
            continue
        items.append(it)
        if it[1] != "more":
            return items
        pos = it[3]


def _walk(eng, fmt, buf, w, file_state=None):
    return (eng.walk_fasta_device if fmt == "fasta" else eng.walk_fastq_device)(buf, w, file_state)


def _assert_generator(eng, fmt, data, buf, w):
    """the generator against the model's walk: item for item the IDs, the lengths, the end and the absolute position"""
    want, _ = walk_model(fmt, data, w)
    got = list(_walk(eng, fmt, buf, w))
    assert [(f.ids, f.lens.tolist(), f.end, f.bad_char, f.end_pos) for f in got] == \
           [([i for i, _ in reads], [len(c) for _, c in reads], end, bad, pos) for reads, end, bad, pos in want]
    return got


def _two_calls(eng, fmt, data, buf, c):
    """a window of c bytes with more behind it, then the rest from its end_pos: both against the model, together against the file"""
    first = _item(_parse(eng, fmt, buf[:c], True))
    assert first == _model_item(fmt, data[:c], True), c
    if first[1] != "more":
        _assert_equivalent(fmt, data, [first])
        return first, None
    rest = _item(_parse(eng, fmt, buf[first[3]:], False), first[3])
    _assert_equivalent(fmt, data, [first, rest])
    return first, rest


# ---- 1: every cut of a file written by hand ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_every_cut_of_a_hand_written_file(eng, fmt):
    data = HAND[fmt]
    buf = _device(data)
    heads, ends = header_windows(data), fourth_lfs(data)
    for c in range(1, len(data)):
        first, rest = _two_calls(eng, fmt, data, buf, c)
        assert first[1] == "more" and rest[1] == "eof"
        if fmt == "fasta":                                          # the first call is maximal
            assert len(first[0]) == max(sum(1 for h in heads if h < c) - 1, 0)
        else:
            assert len(first[0]) == sum(1 for e in ends if e <= c)


# ---- 2: hostile files ------------------------------------------------------------------------------------------------------------------
HOSTILE = [("fasta", k) for k in sorted(FASTA_CASES)] + [("fastq", k) for k in sorted(FASTQ_STOPS)]


@pytest.mark.parametrize("fmt,case", HOSTILE, ids=[f"{f}-{k}" for f, k in HOSTILE])
def test_walks_of_hostile_files_end_on_the_files_own_stop(eng, fmt, case):
    data = FASTA_CASES[case] if fmt == "fasta" else FASTQ_STOPS[case][0]
    buf = _device(data)
    want = whole(fmt, data)
    for w in WALK_WINDOWS:
        items = _parse_walk(eng, fmt, data, buf, w, MAX_CALLS)
        _assert_equivalent(fmt, data, items)                        # every item but the last says "more": no stop the file does not have
        got = _assert_generator(eng, fmt, data, buf, w)
        assert (got[-1].end, got[-1].bad_char, got[-1].end_pos) == want[1:]
        assert all(f.end == "more" for f in got[:-1])


def test_a_cut_quality_line_is_no_format_stop(eng):
    data = FASTQ_STOPS["good"][0]
    buf = _device(data)
    lfs = [i for i in range(len(data)) if data[i] == 10]
    ends = set()
    for k in range(3, len(lfs), 4):                                 # every quality line: cut in it, in front of its LF, behind its LF
        for c in (lfs[k - 1] + 2, lfs[k], lfs[k] + 1):
            f = eng.parse_fastq_device(buf[:c], more=True)
            assert f.end == "more" and len(f.ids) == (k + 1) // 4 - (0 if c > lfs[k] else 1)
            ends.add(eng.parse_fastq_device(buf[:c]).end)           # what the whole-file call says of the same bytes
            assert ends <= {"format", "eof"} and eng.parse_fastq_device(buf[:c]).end == fastq_rules(data[:c])[1]
    assert "format" in ends


# ---- 3: a header window in the middle of a line ----------------------------------------------------------------------------------------
def _seq(rng, n, lower=0.3):
    b = ACGT[rng.randint(0, 4, size=n)].copy()
    b[rng.rand(n) < lower] += 32
    return b.tobytes()


def _wrapped(rng, n, width=60, eol=b"\n"):
    s = _seq(rng, n)
    return eol.join(s[i:i + width] for i in range(0, n, width)) + eol


def test_a_header_window_in_the_middle_of_a_line(eng):
    rng = np.random.RandomState(31)
    pre = b">r0\nACGT\n>r1 the long line\n"
    data = pre + _seq(rng, WINDOW) + b">x in mid line\n" + _wrapped(rng, 300) + b">r3\nAC\n"
    gt = len(pre) + WINDOW                                          # 4095 bytes behind the line start: a window starts here, with '>'
    assert data[gt:gt + 2] == b">x" and b"\n" not in data[len(pre):gt] and header_windows(data)[2] == gt
    assert [i for i, _ in rules(data)[0]] == [b"r0", b"r1 the long line", b"x in mid line", b"r3"]
    buf = _device(data)
    for c in (gt - 1, gt, gt + 1, gt + 2, gt + 20):
        first, rest = _two_calls(eng, "fasta", data, buf, c)
        if c > gt:                                                  # the '>' is in the window: r1 is closed, and the walk resumes on the '>'
            assert [i for i, _ in first[0]] == [b"r0", b"r1 the long line"] and first[3] == gt
            assert rest[0][0][0] == b"x in mid line"
        else:
            assert [i for i, _ in first[0]] == [b"r0"] and first[3] == data.index(b">r1")
    for w in (gt - 1, gt, gt + 1, len(pre) + 10, 1000):
        items = _parse_walk(eng, "fasta", data, buf, w, MAX_CALLS)
        _assert_equivalent("fasta", data, items)
        _assert_generator(eng, "fasta", data, buf, w)
    assert gt in [it[3] for it in _parse_walk(eng, "fasta", data, buf, gt + 1)]


# ---- 4: tile edges ---------------------------------------------------------------------------------------------------------------------
def _fasta_fill(rng, nbytes):
    """nbytes of a record '>a': its header and wrapped lines; the last byte is the LF that ends it"""
    body = nbytes - 3
    out = b">a\n" + _wrapped(rng, body, 60)[:body - 1]
    out = (out[:-1] + b"A" if out.endswith(b"\n") else out) + b"\n"
    assert len(out) == nbytes
    return out


def _fastq_fill(rng, nbytes):
    """nbytes of complete four-line records; the last byte is the fourth LF of the last one"""
    out = b""
    while nbytes - len(out) > 600:
        s = _seq(rng, 100)
        out += b"@f\n" + s + b"\n+\n" + b"I" * 100 + b"\n"
    r = nbytes - len(out)
    ident, n = (b"@f", (r - 7) // 2) if r % 2 else (b"@ff", (r - 8) // 2)
    out += ident + b"\n" + _seq(rng, n) + b"\n+\n" + b"F" * n + b"\n"
    assert len(out) == nbytes and n >= 1
    return out


def _edge_files():
    rng = np.random.RandomState(41)
    out = {}
    for p in (T - 1, T, T + 1):
        # the header's first byte at p (the record before it ends at p - 1); the record's last byte, its LF, at p (the header at p + 1)
        for what, n in (("header", p), ("record_end", p + 1)):
            tail = b">b at the edge\n" + _wrapped(rng, 500) + b">c\n" + _wrapped(rng, T + 100) + b">d\nACGT\n"
            out["fasta", f"{what}_at_{p}"] = _fasta_fill(rng, n) + tail
            s = _seq(rng, 300)
            tail = b"@b at the edge\n" + s + b"\n+\n" + b"I" * 300 + b"\n" + _fastq_fill(rng, T + 100) + b"@d\nACGT\n+\nIIII\n"
            out["fastq", f"{what}_at_{p}"] = _fastq_fill(rng, n) + tail
    return out


EDGE_FILES = _edge_files()


@pytest.mark.parametrize("fmt,name", sorted(EDGE_FILES), ids=[f"{f}-{k}" for f, k in sorted(EDGE_FILES)])
def test_cuts_on_the_tile_edges(eng, fmt, name):
    data = EDGE_FILES[fmt, name]
    p = int(name.rsplit("_", 1)[1])
    if name.startswith("header"):
        assert data[p:p + 2] in (b">b", b"@b") and data[p - 1] == 10
    else:
        assert data[p] == 10 and data[p + 1:p + 3] in (b">b", b"@b")
    buf = _device(data)
    for c in (T - 1, T, T + 1):
        first, rest = _two_calls(eng, fmt, data, buf, c)
        assert first[1] == "more" and rest[1] == "eof"
        head = p if name.startswith("header") else p + 1           # where record b's header line begins
        if fmt == "fastq":
            assert (len(first[0]) > 0 and first[3] == head) == (c >= head)        # the records in front of b, once their last LF is in
        else:
            assert (len(first[0]) == 1 and first[3] == head) == (c > head)        # a, once b's '>' is in
    for w in (T - 1, T, T + 1):
        _assert_equivalent(fmt, data, _parse_walk(eng, fmt, data, buf, w, MAX_CALLS))
        _assert_generator(eng, fmt, data, buf, w)


# ---- 5: a window smaller than a record ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_a_window_smaller_than_a_record_widens(eng, fmt):
    rng = np.random.RandomState(51)
    recs = [(b"r%d of 2 kb" % k, _seq(rng, 2000 + 13 * k, lower=0.0)) for k in range(7)]
    if fmt == "fasta":
        data = b"".join(b">" + i + b"\n" + b"\n".join(s[k:k + 70] for k in range(0, len(s), 70)) + b"\n" for i, s in recs)
    else:
        data = to_fastq(recs)
    buf = _device(data)
    want, calls = walk_model(fmt, data, 64)
    assert len(want) >= 4 and calls > len(want)                     # 64 -> 4096 holds one record and the next header: about a read a batch
    got = _assert_generator(eng, fmt, data, buf, 64)
    assert len(got) == len(want) and got[-1].end == "eof" and got[-1].end_pos == len(data)
    assert [i for f in got for i in f.ids] == [i for i, _ in recs] and [n for f in got for n in f.lens.tolist()] == [len(s) for _, s in recs]
    _assert_equivalent(fmt, data, _parse_walk(eng, fmt, data, buf, 64, MAX_CALLS))


# ---- 6: file bytes in, the reference's stdout bytes out, batch by batch ----------------------------------------------------------------------
def _golden(name, mode):
    p = os.path.join(gu.GOLDEN, f"{name}.{mode}.stdout")
    return open(p, "rb").read() if os.path.exists(p) else None


def _stdout_of_a_walk(eng, items, with_a):
    """run and report between the items of a walk: (stdout, -a stdout, batches, the items)"""
    out, out_a, n, seen = b"", b"", 0, []
    for f in items:
        seen.append(f)
        if len(f.ids) == 0:
            continue                                                # nothing is resident
        eng.run()
        out += eng.report_bytes(f.ids)
        if with_a:
            out_a += eng.report_bytes(f.ids, alignments=True)
        n += 1
    return out, out_a, n, seen


def _upload_window(eng, fmt, buf, more_follows, file_state=None):
    """mtr_upload_*_device_window through ctypes, as upload_*_device does it: more_follows = 0 goes to the _window entry point too"""
    info = mtr_amd.CFastaInfo()
    torch.cuda.synchronize()
    entry = f"mtr_upload_{fmt}_device_window"
    eng.n_reads = 0
    eng._check(getattr(eng.lib, entry)(eng.h, file_state.h if file_state is not None else None, C.c_void_p(buf.data_ptr()), buf.numel(), more_follows,
                                       None, C.byref(info)), entry)
    eng.n_reads = info.n_reads
    return info


@pytest.mark.parametrize("name", ["3_5", "edge", "synth_c2"])
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_file_bytes_in_stdout_bytes_out_in_batches(eng, fmt, name):
    raw = golden_raw(name)
    data = raw if fmt == "fasta" else golden_fastq(raw)
    buf = _device(data)
    want, want_a = _golden(name, "default"), _golden(name, "a")
    out, out_a, n, seen = _stdout_of_a_walk(eng, _walk(eng, fmt, buf, len(data) // 4), want_a is not None)
    model, _ = walk_model(fmt, data, len(data) // 4)
    assert [(f.ids, f.end, f.end_pos) for f in seen] == [([i for i, _ in reads], end, pos) for reads, end, _, pos in model]
    assert n == 1 if name == "3_5" else n >= 3                      # 3_5 is one record: its walk widens to the file
    assert out == want and (want_a is None or out_a == want_a)
    # one window over the file: more_follows = 0 through the _window entry point is the entry point without _window
    ids = [i for i, _ in whole(fmt, data)[0]]
    info = _upload_window(eng, fmt, buf, 0)
    assert (info.n_reads, info.end, info.end_pos) == (len(ids), 0, len(data))
    eng.run()
    assert eng.report_bytes(ids) == want and (want_a is None or eng.report_bytes(ids, alignments=True) == want_a)
    twin = (eng.upload_fasta_device if fmt == "fasta" else eng.upload_fastq_device)(buf)
    assert (twin.ids, twin.end, twin.end_pos) == (ids, "eof", len(data))


# ---- 7: file-order mode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_lengths", "stale_org_base"])
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_file_order_walk_equals_the_capture(eng, fmt, name):
    raw = golden_raw(name)
    data = raw if fmt == "fasta" else golden_fastq(raw)
    want = _capture(name)
    fs = mtr_amd.FileState()
    ranges, got, ids, out_a, n = [], [], [], b"", 0
    for f in _walk(eng, fmt, _device(data), len(data) // 4, fs):
        if len(f.ids) == 0:
            continue
        ranges += eng.test_ranges()
        eng.run()
        got += _rec(eng.fetch())
        ids += f.ids
        if name == "stale_org_base":
            out_a += eng.report_bytes(f.ids, alignments=True)
        n += 1
    fs.close()
    assert n >= 3 and len(ids) == len(want) and f.end == "eof" and f.end_pos == len(data)
    for i in range(len(want)):
        assert ranges[i] == want[i][0], f"read {i}: ranges differ"
        assert got[i] == want[i][1], f"read {i}: records differ"
    if name == "stale_org_base":
        assert out_a == open(os.path.join(FO, "stale_org_base.a.stdout"), "rb").read()


# ---- 8: refusals through the C-ABI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_library_refuses_a_bad_mode_and_a_small_destination(eng, fmt):
    lib, data = eng.lib, HAND[fmt]
    t = _device(data)
    info = mtr_amd.CFastaInfo()
    parse, upload = getattr(lib, f"mtr_parse_{fmt}_device_window"), getattr(lib, f"mtr_upload_{fmt}_device_window")
    torch.cuda.synchronize()
    eng.upload([np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 80)])          # a batch that a refused mode must leave alone
    for bad in (2, -1, 256):
        assert parse(eng.h, C.c_void_p(t.data_ptr()), len(data), bad, None, None, C.byref(info)) == 2
        assert "more_follows" in lib.mtr_last_error(eng.h).decode()
        assert upload(eng.h, None, C.c_void_p(t.data_ptr()), len(data), bad, None, C.byref(info)) == 2
    eng.run()
    assert len(eng.fetch()[0]) >= 1
    # n_bytes == 0 with more behind it: no reads, "more", end_pos 0 - and no pointer is looked at
    for ptr in (None, C.c_void_p(t.data_ptr())):
        info = mtr_amd.CFastaInfo(7, 7, 7, 7, 7, 7, 7)
        assert parse(eng.h, ptr, 0, 1, None, None, C.byref(info)) == 0
        assert (info.n_reads, info.end, info.end_pos, info.n_bases, info.id_bytes) == (0, 5, 0, 0, 0)
        info = mtr_amd.CFastaInfo(7, 7, 7, 7, 7, 7, 7)
        assert upload(eng.h, None, ptr, 0, 1, None, C.byref(info)) == 0
        assert (info.n_reads, info.end, info.end_pos) == (0, 5, 0)
    f = _parse(eng, fmt, t[:0], True)
    assert (f.ids, f.end, f.end_pos) == ([], "more", 0)
    # sizes only, then every capacity one below them: MTR_ERR_OVERFLOW, the sizes filled in, not a byte written
    c = len(data) - 3
    reads, end, _, pos = window_model(fmt, data[:c], True)
    assert end == "more" and len(reads) >= 4
    assert parse(eng.h, C.c_void_p(t.data_ptr()), c, 1, None, None, C.byref(info)) == 0
    n, nb, ni = info.n_reads, info.n_bases, info.id_bytes
    assert (n, nb, ni, info.end, info.end_pos) == (len(reads), sum(len(x) for _, x in reads), sum(len(i) for i, _ in reads), 5, pos)
    cols = [torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((n,), -7, dtype=torch.int64, device="cuda"),
            torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((ni,), 0x5A, dtype=torch.uint8, device="cuda"),
            torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")]
    before = [x.clone() for x in cols]
    torch.cuda.synchronize()
    for caps in ((nb - 1, n, ni), (nb, n - 1, ni), (nb, n, ni - 1)):
        info = mtr_amd.CFastaInfo()
        dst = mtr_amd.CFastaDst(*[x.data_ptr() for x in cols], *caps)
        assert parse(eng.h, C.c_void_p(t.data_ptr()), c, 1, None, C.byref(dst), C.byref(info)) == 5 and "needed" in lib.mtr_last_error(eng.h).decode()
        assert (info.n_reads, info.n_bases, info.id_bytes, info.end, info.end_pos) == (n, nb, ni, 5, pos)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(cols, before))
    dst = mtr_amd.CFastaDst(*[x.data_ptr() for x in cols], nb, n, ni)
    assert parse(eng.h, C.c_void_p(t.data_ptr()), c, 1, None, C.byref(dst), C.byref(info)) == 0
    assert cols[2].tolist() == [len(x) for _, x in reads] and cols[4].tolist()[-1] == ni
    assert cols[3].cpu().numpy().tobytes() == b"".join(i for i, _ in reads)
    with pytest.raises(mtr_amd.MtrError, match="window_bytes"):
        next(iter(eng.walk_fasta_device(t, 0)))
