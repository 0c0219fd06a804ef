"""A FASTA or FASTQ file in device memory walked batch by batch (mtr_parse_fasta_device_window / mtr_upload_fasta_device_window and
their FASTQ twins, Engine.walk_fasta_device / walk_fastq_device) on the CPU: the header declares the entry points, the library exports
them, the walk methods refuse bad arguments before the library is called - and window_model / walk_model, the window rules of
include/mtr_hip.h restated in Python over rules() and fastq_rules(), with the files and the claims that
tests/test_gpu_walk_device.py makes about them checked here, where no GPU is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd
from mtr_amd import build as mbuild
from tests import golden_util as gu
from tests.test_fastq_device import LUT, MAX_INPUT_LENGTH, fastq_lines, fastq_rules, to_fastq
from tests.test_host_driver import FASTA_CASES, reference_reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mtr_parse_fasta_device_window", "mtr_upload_fasta_device_window", "mtr_parse_fastq_device_window", "mtr_upload_fastq_device_window")
WINDOW = 4095
ACGT = np.frombuffer(b"ACGT", np.uint8).copy()
FO = os.path.join(gu.GOLDEN, "file_order")


def fasta_rules(data: bytes):
    """rules() of tests/test_gpu_fasta_device.py; that module needs torch at import, this one must not"""
    from tests.test_gpu_fasta_device import rules
    return rules(data)


# ---- the window rules, from their text ---------------------------------------------------------------------------------------------
def header_windows(data: bytes):
    """where the header windows begin: the fgets windows of 4095 bytes - from a line start, cut behind an LF - whose first byte is '>'"""
    out, pos = [], 0
    while pos < len(data):
        nl = data.find(b"\n", pos, pos + WINDOW)
        if data[pos:pos + 1] == b">":
            out.append(pos)
        pos = nl + 1 if nl >= 0 else pos + WINDOW
    return out


def fourth_lfs(data: bytes):
    """the positions behind every fourth LF: where the complete FASTQ records end"""
    lfs = [i + 1 for i in range(len(data)) if data[i] == 10]
    return lfs[3::4]


def window_model(fmt: str, data: bytes, more: bool):
    """([(id, codes)], end, bad_char, end_pos) of one parse call on data; more: the input goes on behind data"""
    if not more:
        return fasta_rules(data) if fmt == "fasta" else fastq_rules(data)
    n = len(data)
    if n == 0:
        return [], "more", None, 0
    if fmt == "fasta":
        reads, end, bad, pos = fasta_rules(data)
        if end in ("bad", "toolong") or (end == "empty" and pos < n):      # a stop in front of the end: the bytes before it decide it
            return reads, end, bad, pos
        heads = header_windows(data)
        k = max(len(heads) - 1, 0)
        return reads[:k], "more", None, heads[-1] if k > 0 else 0
    ends = fourth_lfs(data)
    done = ends[-1] if ends else 0
    reads, end, bad, pos = fastq_rules(data[:done]) if done else ([], "eof", None, 0)
    if end != "eof":                                                      # complete records: every stop in them is decided
        return reads, end, bad, pos
    # the open record: what its lines' first bytes and its sequence's bytes decide
    lines = [(done + s, done + e) for s, e in fastq_lines(data[done:])]
    if lines:
        s, e = lines[0]
        if data[s:s + 1] != b"@":
            return reads, "format", None, s
    if len(lines) > 1:
        s, e = lines[1]
        if e == s:
            return reads, "empty", None, s
        codes = LUT[np.frombuffer(data[s:e], np.uint8)]
        bad_at = np.flatnonzero(codes == 255)
        good = int(bad_at[0]) if len(bad_at) else len(codes)
        if good >= MAX_INPUT_LENGTH:
            return reads, "toolong", None, s + MAX_INPUT_LENGTH - 1
        if len(bad_at):
            return reads, "bad", data[s + good:s + good + 1], s + good
    if len(lines) > 2:
        s, e = lines[2]
        if data[s:s + 1] != b"+":
            return reads, "format", None, s
    return reads, "more", None, done


def walk_model(fmt: str, data: bytes, window_bytes: int, max_calls=None):
    """Engine.walk_*_device by its docstring, over window_model: ([items], calls), an item = (reads, end, bad_char, absolute end_pos)"""
    items, pos, w, calls = [], 0, window_bytes, 0
    while True:
        k = min(w, len(data) - pos)
        reads, end, bad, end_pos = window_model(fmt, data[pos:pos + k], pos + k < len(data))
        calls += 1
        assert max_calls is None or calls <= max_calls
        if end == "more" and not reads:
            w *= 2
            continue
        items.append((reads, end, bad, pos + end_pos))
        if end != "more":
            return items, calls
        pos += end_pos


def joined(items):
    return [(i, np.asarray(c).tolist()) for reads, _, _, _ in items for i, c in reads]


def whole(fmt: str, data: bytes):
    reads, end, bad, pos = window_model(fmt, data, False)
    return [(i, np.asarray(c).tolist()) for i, c in reads], end, bad, pos


def assert_walk_equivalence(fmt, data, items):
    """the contract: the reads over the walk, and the last item's end, are the whole file's; every earlier item says "more" """
    reads, end, bad, pos = whole(fmt, data)
    assert joined(items) == reads
    assert items[-1][1:] == (end, bad, pos)
    assert all(it[1] == "more" for it in items[:-1])


# ---- the files of test 1: written by hand ------------------------------------------------------------------------------------------
# bases in front of the first header; an ID with spaces; a CRLF record; a record of several lines; a lower-case read; a last line
# without its end
HAND_FASTA = (b"ACGTTGCA\nGG\n>first one  with  spaces \nACGTACGTAC\n>crlf\r\nTTAGGGTTAGGG\r\nTTAGGG\r\n>multi\nACGT\nAC\n\nGGTTAACC\nT\n"
              b">lower case\nacgtacgtttgacca\n>mixed Case\nAcGtTTgaCC\nGATTACA\n>last\nCCCCGGGGAAAATTTTCCCCGGGGAAAATTTT\nCAGCAGCAGCAGCAGCAGCAGCAGCAG")
# an ID with spaces; CRLF lines; a lower-case read; a quality line that begins with '@' and one with '+'; an empty ID; a separator that
# repeats the ID; a last line without its end.  (Strict four-line FASTQ has no record of several lines: the sequences differ in length.)
HAND_FASTQ = (b"@first one  with  spaces \nACGTACGTAC\n+\nIIIIIIIIII\n@crlf\r\nTTAGGGTTAGGG\r\n+crlf\r\n@IIIIIIIIIII\r\n"
              b"@lower case\nacgtacgtttgacca\n+\n+FFFFFFFFFFFFFF\n@\nG\n+\n!\n@mixed Case\nAcGtTTgaCCGATTACA\n+mixed Case\n>>>>>>>>>>>>>>>>>\n"
              b"@last\nCCCCGGGGAAAATTTT\n+\nJJJJJJJJJJJJJJJJ")
HAND = {"fasta": HAND_FASTA, "fastq": HAND_FASTQ}

# the stops of FASTQ for test 2 (FASTA's are FASTA_CASES): name -> (file, end of the whole file)
FASTQ_STOPS = {
    "good": (HAND_FASTQ, "eof"),
    "bad_character": (b"@a\nACGT\n+\nIIII\n@b\nACNGT\n+\nIIIII\n@c\nAC\n+\nII\n", "bad"),
    "empty_sequence": (b"@a\nACGT\n+\nIIII\n@b\n\n+\n\n@c\nAC\n+\nII\n", "empty"),
    "header_without_at": (b"@a\nACGT\n+\nIIII\n>b\nACGT\n+\nIIII\n", "format"),
    "separator_without_plus": (b"@a\nACGT\n+\nIIII\n@b\nACGT\n-\nIIII\n", "format"),
    "quality_shorter": (b"@a\nACGT\n+\nIIII\n@b\nACGTACGT\n+\nIIIIIII\n@c\nAC\n+\nII\n", "format"),
    "quality_longer": (b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIIIII\n@c\nAC\n+\nII\n", "format"),
    "cut_inside_a_record": (b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\n", "format"),
    "cut_inside_a_sequence": (b"@a\nACGT\n+\nIIII\n@b\nAC", "format"),
    "trailing_blank_line": (b"@a\nACGT\n+\nIIII\n\n", "format"),
    "long_lines": (b"@a " + b"i" * 5000 + b"\n" + b"ACGT" * 1200 + b"\n+\n" + b"I" * 4800 + b"\n@b\nAC\n+\nII\n", "eof"),
}
WALK_WINDOWS = (1, 2, 17, 4095, 4096, 4097)


def golden_fastq(raw: bytes) -> bytes:
    reads, end = reference_reader(raw)
    assert end == "eof"
    return to_fastq([(i, ACGT[np.asarray(c, np.uint8)].tobytes()) for i, c in reads], repeat_id=True)


def golden_raw(name: str) -> bytes:
    path = os.path.join(FO, name + ".fa") if name in ("mixed_lengths", "stale_org_base") else gu.input_path(name)
    return open(path, "rb").read()


# ---- the claims of the GPU tests, checked on the model -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_hand_files_hold_what_they_claim(fmt):
    data = HAND[fmt]
    reads, end, _, pos = whole(fmt, data)
    assert (end, pos) == ("eof", len(data)) and 5 <= len(reads) <= 6 and 200 <= len(data) <= 500
    ids = [i for i, _ in reads]
    assert any(b"  " in i for i in ids) and b"\r\n" in data
    assert any(bytes(ACGT[np.asarray(c, np.uint8)]).lower() in data for _, c in reads)              # a lower-case read, as written
    if fmt == "fasta":
        assert header_windows(data)[0] == 12 and reads[0][1][:8] == [0, 1, 2, 3, 3, 2, 1, 0]          # bases in front of the first header
        assert reads[2] == (b"multi", LUT[np.frombuffer(b"ACGTACGGTTAACCT", np.uint8)].tolist())


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_model_every_cut_of_the_hand_files(fmt):
    """test 1 on the model: a window and the rest behind its end_pos give the whole file, and the window is maximal"""
    data = HAND[fmt]
    for c in range(1, len(data)):
        reads, end, bad, pos = window_model(fmt, data[:c], True)
        assert end == "more" and pos <= c                          # (the hand files have no stop)
        if fmt == "fasta":
            assert len(reads) == max(sum(1 for h in header_windows(data) if h < c) - 1, 0)
        else:
            assert len(reads) == sum(1 for e in fourth_lfs(data) if e <= c)
        rest = window_model(fmt, data[pos:], False)
        assert_walk_equivalence(fmt, data, [(reads, end, bad, pos), (rest[0], rest[1], rest[2], pos + rest[3])])


def test_model_walks_of_the_hostile_files():
    """test 2 on the model: every stop kind occurs, and every walk ends on the whole file's stop"""
    kinds = {"fasta": set(), "fastq": set()}
    for fmt, cases in (("fasta", FASTA_CASES), ("fastq", {k: v[0] for k, v in FASTQ_STOPS.items()})):
        for name, data in cases.items():
            kinds[fmt].add(whole(fmt, data)[1])
            if fmt == "fastq":
                assert whole(fmt, data)[1] == FASTQ_STOPS[name][1], name
            for w in WALK_WINDOWS:
                items, _ = walk_model(fmt, data, w)
                assert_walk_equivalence(fmt, data, items)
    assert kinds["fasta"] == {"eof", "empty", "bad"}               # (the reader's limit of 1 000 000 bases is test_model_toolong's)
    assert kinds["fastq"] == {"eof", "empty", "bad", "format"}


def test_model_toolong():
    data = b">ok\nACGT\n>huge\n" + b"ACGTACGTAC" * 100001 + b"\n>never\nAC\n"
    for w in (300000, 1 << 20):
        items, _ = walk_model("fasta", data, w)
        assert_walk_equivalence("fasta", data, items)
        assert items[-1][1] == "toolong"


@pytest.mark.parametrize("name", ["3_5", "edge", "synth_c2", "mixed_lengths", "stale_org_base"])
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_model_goldens_walk_in_three_batches(fmt, name):
    """tests 6 and 7 on the model: a quarter of the file as the window gives three batches or more.  3_5 is one record: its walk is
    the widening case, one batch."""
    raw = golden_raw(name)
    data = raw if fmt == "fasta" else golden_fastq(raw)
    items, _ = walk_model(fmt, data, len(data) // 4)
    assert_walk_equivalence(fmt, data, items)
    assert len(items) == 1 if name == "3_5" else len(items) >= 3


# ---- the header, the library, the mirror -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return mtr_amd.load_library()


def test_header_declares_the_entry_points_and_keeps_its_version():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtr_hip.h")).read(), flags=re.S)
    assert re.search(r"^#define MTR_ABI_VERSION 5\b", hdr, flags=re.M)
    assert re.search(r"^#define MTR_FASTA_END_MORE 5\b", hdr, flags=re.M)
    args = {name: [a.strip().split()[-1].lstrip("*") for a in re.search(rf"mtr_status\s+{name}\s*\(([^)]*)\)", hdr).group(1).split(",")] for name in NAMES}
    assert args["mtr_parse_fasta_device_window"] == ["ctx", "d_fasta", "n_bytes", "more_follows", "wait_stream", "dst", "info"]
    assert args["mtr_upload_fasta_device_window"] == ["ctx", "fs", "d_fasta", "n_bytes", "more_follows", "wait_stream", "info"]
    assert args["mtr_parse_fastq_device_window"] == ["ctx", "d_fastq", "n_bytes", "more_follows", "wait_stream", "dst", "info"]
    assert args["mtr_upload_fastq_device_window"] == ["ctx", "fs", "d_fastq", "n_bytes", "more_follows", "wait_stream", "info"]


def test_the_mirror_names_the_new_end_and_exports():
    assert set(NAMES) <= set(mtr_amd.EXPORTS)
    assert mtr_amd.FASTQ_END[5] == "more" and mtr_amd.FASTQ_END[4] == "format"
    assert mtr_amd.FASTA_END == {0: "eof", 1: "empty", 2: "bad", 3: "toolong"}
    assert {k: mtr_amd.FASTQ_END[k] for k in mtr_amd.FASTA_END} == mtr_amd.FASTA_END


def test_library_exports_the_entry_points(lib):
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.mtr_abi_version() == 5
    info = mtr_amd.CFastaInfo()
    for more in (0, 1):
        assert lib.mtr_parse_fasta_device_window(None, C.c_void_p(0x1000), 16, more, None, None, C.byref(info)) == 2      # MTR_ERR_BAD_ARG
        assert lib.mtr_parse_fastq_device_window(None, C.c_void_p(0x1000), 16, more, None, None, C.byref(info)) == 2
        assert lib.mtr_upload_fasta_device_window(None, None, C.c_void_p(0x1000), 16, more, None, C.byref(info)) == 2
        assert lib.mtr_upload_fastq_device_window(None, None, C.c_void_p(0x1000), 16, more, None, C.byref(info)) == 2


@pytest.mark.parametrize("method", ["walk_fasta_device", "walk_fastq_device"])
def test_walk_methods_refuse_bad_arguments_before_the_library_is_called(method):
    torch = pytest.importorskip("torch")
    e = mtr_amd.Engine.__new__(mtr_amd.Engine)                  # no context: the checks must raise before anything is called
    e.h, e.lib, e.device = None, None, 0
    call = getattr(e, method)                                    # the checks are made by the call, not by the first next() on its result
    with pytest.raises(mtr_amd.MtrError, match="torch.Tensor"):
        call(np.zeros(64, np.uint8), 16)
    with pytest.raises(mtr_amd.MtrError, match="torch.Tensor"):
        call(b">r\nACGT\n", 16)
    with pytest.raises(mtr_amd.MtrError, match="torch.uint8"):
        call(torch.zeros(64, dtype=torch.int8), 16)
    with pytest.raises(mtr_amd.MtrError, match="contiguous"):
        call(torch.zeros(128, dtype=torch.uint8)[::2], 16)
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):
        call(torch.zeros(64, dtype=torch.uint8), 16)
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(mtr_amd.MtrError, match="window_bytes"):
            call(torch.zeros(64, dtype=torch.uint8), bad)


@pytest.mark.parametrize("method", ["parse_fasta_device", "parse_fastq_device", "upload_fasta_device", "upload_fastq_device"])
def test_more_is_checked_like_a_whole_file(method):
    torch = pytest.importorskip("torch")
    e = mtr_amd.Engine.__new__(mtr_amd.Engine)
    e.h, e.lib, e.device = None, None, 0
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):
        getattr(e, method)(torch.zeros(64, dtype=torch.uint8), more=True)
