"""A FASTQ file in device memory (mtr_parse_fastq_device / mtr_upload_fastq_device / mtr_upload_fastq_device_in_file,
Engine.parse_fastq_device / upload_fastq_device) on the CPU: the header declares the entry points, the library exports them, the
argument checks refuse bad tensors before the library is called - and fastq_rules, the rules of include/mtr_hip.h restated in
Python, which tests/test_gpu_fastq_device.py holds the kernels against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd
from mtr_amd import build as mbuild
from tests.test_host_driver import reference_reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mtr_parse_fastq_device", "mtr_upload_fastq_device", "mtr_upload_fastq_device_in_file")
MAX_INPUT_LENGTH = 1000000
LUT = np.full(256, 255, np.uint8)
for _c, _v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
    LUT[_c] = _v


# ---- the rules, from their text ----------------------------------------------------------------------------------------------
def fastq_lines(data: bytes):
    """[(start, content_end)]: line 0 starts at byte 0, line l + 1 behind the l-th LF if a byte exists there; the content ends in
    front of the line's first NUL, LF or CR, or with the line"""
    out, start = [], 0
    while start < len(data):
        lf = data.find(b"\n", start)
        stop = len(data) if lf < 0 else lf + 1
        end = stop
        for t in (b"\0", b"\n", b"\r"):
            k = data.find(t, start, end)
            if k >= 0:
                end = k
        out.append((start, end))
        start = stop
    return out


def fastq_rules(data: bytes):
    """([(id, codes)], end, bad_char, end_pos): the reads before the first stop in file order, and the stop"""
    n = len(data)
    if n == 0:
        return [], "empty", None, 0
    lines, reads = fastq_lines(data), []
    for at in range(0, len(lines), 4):
        rec = lines[at:at + 4]
        s, e = rec[0]
        if data[s:e][:1] != b"@":
            return reads, "format", None, s
        ident = data[s + 1:e]
        if len(rec) < 2:
            return reads, "format", None, n
        s, e = rec[1]
        if e == s:
            return reads, "empty", None, s
        codes = LUT[np.frombuffer(data[s:e], np.uint8)]
        bad = np.flatnonzero(codes == 255)
        good = int(bad[0]) if len(bad) else len(codes)
        if good >= MAX_INPUT_LENGTH:
            return reads, "toolong", None, s + MAX_INPUT_LENGTH - 1
        if len(bad):
            return reads, "bad", data[s + good:s + good + 1], s + good
        if len(rec) < 3:
            return reads, "format", None, n
        s, e = rec[2]
        if data[s:e][:1] != b"+":
            return reads, "format", None, s
        if len(rec) < 4:
            return reads, "format", None, n
        s, e = rec[3]
        if e - s != len(codes):
            return reads, "format", None, s
        reads.append((ident, codes))
    return reads, "eof", None, n


def to_fastq(records, eol=b"\n", last_eol=True, repeat_id=False, quals=None) -> bytes:
    """records [(id, sequence)] as four-line FASTQ; quals: per record its quality line (default 'I' per base); repeat_id: the
    separator repeats the ID; last_eol False: the last quality line has no line end"""
    out = []
    for k, (ident, seq) in enumerate(records):
        q = quals[k] if quals is not None else b"I" * len(seq)
        out += [b"@" + ident, eol, seq, eol, b"+" + (ident if repeat_id else b""), eol, q, eol]
    if out and not last_eol:
        out.pop()
    return b"".join(out)


def to_fasta(records) -> bytes:
    return b"".join(b">" + ident + b"\n" + seq + b"\n" for ident, seq in records)


def random_records(rng, n, lo=1, hi=300, lower=0.3):
    recs = []
    for k in range(n):
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, rng.randint(lo, hi + 1))]
        seq = np.where(rng.rand(len(seq)) < lower, seq | 0x20, seq).astype(np.uint8).tobytes()
        recs.append((b"read %d len=%d" % (k, len(seq)), seq))
    return recs


# ---- the rules against themselves and against the FASTA reader ------------------------------------------------------------------------
@pytest.mark.parametrize("eol,last_eol,repeat_id", [(b"\n", True, False), (b"\r\n", True, True), (b"\n", False, False), (b"\r\n", False, True)])
def test_rules_read_back_what_to_fastq_writes(eol, last_eol, repeat_id):
    rng = np.random.RandomState(11)
    recs = random_records(rng, 50) + [(b"", b"acgt"), (b" spaces  kept ", b"T")]
    quals = [bytes(rng.randint(33, 127, len(s)).astype(np.uint8)) for _, s in recs]       # '@', '>' and '+' among them
    quals[3] = b"@" + quals[3][1:]
    quals[4] = b"+" + quals[4][1:]
    quals[5] = b">" + quals[5][1:]
    data = to_fastq(recs, eol, last_eol, repeat_id, quals)
    reads, end, bad, pos = fastq_rules(data)
    assert (end, bad, pos) == ("eof", None, len(data))
    assert [i for i, _ in reads] == [i for i, _ in recs]
    assert [c.tolist() for _, c in reads] == [LUT[np.frombuffer(s, np.uint8)].tolist() for _, s in recs]


def test_rules_agree_with_the_fasta_reader_on_the_same_records():
    recs = random_records(np.random.RandomState(12), 80)
    reads, end, _, _ = fastq_rules(to_fastq(recs))
    ref_reads, ref_end = reference_reader(to_fasta(recs))
    assert end == ref_end == "eof"
    assert [(i, c.tolist()) for i, c in reads] == [(i, list(c)) for i, c in ref_reads]


@pytest.mark.parametrize("data,want", [
    (b"", (0, "empty", None, 0)),
    (b"@a\nAC\n+\nII\n", (1, "eof", None, 11)),
    (b"@a\nAC\n+\nII", (1, "eof", None, 10)),
    (b"@a\nAC\n+\nII\n\n", (1, "format", None, 11)),                  # a trailing blank line: a header line without '@'
    (b"@a\nAC\n+\nII\n@b\nANT\n+\nIII\n", (1, "bad", b"N", 15)),
    (b"@a\nAC\n+\nII\n@b\n\n+\n\n", (1, "empty", None, 14)),
    (b"@a\nAC\n+\nII\n>b\nAC\n+\nII\n", (1, "format", None, 11)),
    (b"@a\nAC\n-\nII\n", (0, "format", None, 6)),
    (b"@a\nAC\n+\nI\n", (0, "format", None, 8)),
    (b"@a\nAC\n+\nIII\n", (0, "format", None, 8)),
    (b"@a\nAC\n+\nI\0I\n", (0, "format", None, 8)),                   # a NUL hides the rest of the quality line
    (b"@a\n", (0, "format", None, 3)),
    (b"@a\nAC\n", (0, "format", None, 6)),
    (b"@a\nAC\n+\n", (0, "format", None, 8)),
    (b"@a\0b\nAC\r\n+a\n@>\n", (1, "eof", None, 15)),
])
def test_rules_on_files_read_by_hand(data, want):
    reads, end, bad, pos = fastq_rules(data)
    assert (len(reads), end, bad, pos) == want
    if data.startswith(b"@a\0b"):
        assert reads[0][0] == b"a" and reads[0][1].tolist() == [0, 1]


# ---- the header, the library, the mirror ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return mtr_amd.load_library()


def test_header_declares_the_entry_points_and_keeps_its_version():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtr_hip.h")).read(), flags=re.S)
    assert re.search(r"^#define MTR_ABI_VERSION 5\b", hdr, flags=re.M)
    assert re.search(r"^#define MTR_FASTA_END_FORMAT 4\b", hdr, flags=re.M)
    args = {name: [a.strip().split()[-1].lstrip("*") for a in re.search(rf"mtr_status\s+{name}\s*\(([^)]*)\)", hdr).group(1).split(",")] for name in NAMES}
    assert args["mtr_parse_fastq_device"] == ["ctx", "d_fastq", "n_bytes", "wait_stream", "dst", "info"]
    assert args["mtr_upload_fastq_device"] == ["ctx", "d_fastq", "n_bytes", "wait_stream", "info"]
    assert args["mtr_upload_fastq_device_in_file"] == ["ctx", "fs", "d_fastq", "n_bytes", "wait_stream", "info"]


def test_the_mirror_names_the_new_end_and_exports():
    assert set(NAMES) <= set(mtr_amd.EXPORTS)
    assert mtr_amd.FASTQ_END[4] == "format"
    assert {k: mtr_amd.FASTQ_END[k] for k in mtr_amd.FASTA_END} == mtr_amd.FASTA_END       # the four ends FASTA has keep their names
    assert "fastq.hip.inc" in mbuild.SOURCES


def test_library_exports_the_entry_points(lib):
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.mtr_abi_version() == 5
    info = mtr_amd.CFastaInfo()
    assert lib.mtr_parse_fastq_device(None, C.c_void_p(0x1000), 16, None, None, C.byref(info)) == 2      # MTR_ERR_BAD_ARG
    assert lib.mtr_upload_fastq_device(None, C.c_void_p(0x1000), 16, None, C.byref(info)) == 2
    assert lib.mtr_upload_fastq_device_in_file(None, None, C.c_void_p(0x1000), 16, None, C.byref(info)) == 2


@pytest.mark.parametrize("method", ["parse_fastq_device", "upload_fastq_device"])
def test_methods_refuse_bad_buffers_before_the_library_is_called(method):
    torch = pytest.importorskip("torch")
    e = mtr_amd.Engine.__new__(mtr_amd.Engine)                  # no context: the checks must raise before anything is called
    e.h, e.lib, e.device = None, None, 0
    call = getattr(e, method)
    with pytest.raises(mtr_amd.MtrError, match="torch.Tensor"):
        call(np.zeros(64, np.uint8))
    with pytest.raises(mtr_amd.MtrError, match="torch.Tensor"):
        call(b"@r\nACGT\n+\nIIII\n")
    with pytest.raises(mtr_amd.MtrError, match="torch.uint8"):
        call(torch.zeros(64, dtype=torch.int8))
    with pytest.raises(mtr_amd.MtrError, match="contiguous"):
        call(torch.zeros(128, dtype=torch.uint8)[::2])
    with pytest.raises(mtr_amd.MtrError, match="1-D"):
        call(torch.zeros(8, 8, dtype=torch.uint8))
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):
        call(torch.zeros(64, dtype=torch.uint8))
