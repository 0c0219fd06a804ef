"""The report as text (mtr_report_text_device, Engine.report_text / report_bytes) without a device: the Python wrapper's argument
checks, the ID packing, the declarations - and the oracle of the GPU fuzz (tests/test_gpu_report_text.py): the rows of fuzz_rows()
printed by format_report are what C prints, the ratio by glibc's snprintf("%f") through ctypes, the integers by "%d".
tests/test_report_format.py pins format_report to print.c on eleven canned records; here are the values it has not: negative and
extreme integers, quotients above 1 and below 0, exact halfway points of the sixth decimal, infinities of both signs, -0.0."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
RATIO_NAN_BITS = 0xffc00000          # what the ratio column holds for 0 / 0 (chain.hip.inc: report_ratio): the NaN an x86 host makes

# (num_matches, repeat_len) -> the ratio mTR prints
PINNED = [(1, 128, "0.007812"), (3, 128, "0.023438"), (5, 128, "0.039062"), (7, 128, "0.054688"),      # exact halves: to even
          (1, 2 ** 20, "0.000001"), (1, 2 ** 21, "0.000000"), (3, 2 ** 21, "0.000001"), (1, 2 ** 30, "0.000000"),
          (7, 2, "3.500000"), (1000, 3, "333.333344"), (INT_MAX, 1, "2147483648.000000"), (2 ** 24 + 1, 1, "16777216.000000"),
          (-1, 128, "-0.007812"), (-3, 128, "-0.023438"), (-7, 2, "-3.500000"), (5, -3, "-1.666667"), (INT_MIN, 1, "-2147483648.000000"),
          (INT_MIN, INT_MIN, "1.000000"), (INT_MIN, INT_MAX, "-1.000000"), (0, -5, "-0.000000"), (0, 7, "0.000000"),
          (5, 0, "inf"), (0, 0, "-nan"), (-5, 0, "-inf"), (INT_MAX, 0, "inf"), (INT_MIN, 0, "-inf")]


def fuzz_rows(seed=20261, n=6000):
    """(fields int32 [n, 14], read_len int32 [n], units [bytes], ids [bytes or str]) for mtr_test_report_lines.
    Every integer column draws from all magnitudes and both signs and, one time in four, from 0, +-1, INT_MIN, INT_MAX and the powers
    of ten's neighbours.  rep_start and rep_end stop at INT_MAX - 1: the line prints them plus one, and C's int does not go further.
    The first rows are PINNED; units have 0, 1, 499 and other lengths; IDs are empty, short, long, with blanks, and non-ASCII."""
    rng = np.random.RandomState(seed)
    special = np.array([0, 1, -1, INT_MIN, INT_MAX, 9, 10, 99, 100, -100, 999999, 1000000, -1000000, 2 ** 24, 2 ** 24 + 1, 128, 50], np.int64)
    mag = rng.randint(0, 2 ** 31, size=(n, 15)).astype(np.int64) >> rng.randint(0, 31, size=(n, 15))
    val = np.where(rng.randint(0, 2, size=(n, 15)) == 1, -mag, mag)
    val = np.where(rng.randint(0, 4, size=(n, 15)) == 0, special[rng.randint(0, len(special), size=(n, 15))], val)
    pow2 = rng.randint(0, 3, size=n) == 0                        # a third of the rows divide by a power of two: short expansions, many halves
    val[pow2, 2] = 1 << rng.randint(0, 31, size=int(pow2.sum()))
    for k, (m, ln, _) in enumerate(PINNED):
        val[k, 5], val[k, 2] = m, ln
    val[:, 0:2] = np.minimum(val[:, 0:2], INT_MAX - 1)
    fields, read_len = val[:, :14].astype(np.int32), val[:, 14].astype(np.int32)
    ulen = rng.choice([0, 1, 499, 2, 3, 7, 31, 64, 200], size=n)
    units = [b"ACGT"[0:0].join(bytes([b"ACGT"[c]]) for c in rng.randint(0, 4, size=int(u))) for u in ulen]
    kinds = [b"", b"r", b"read 7 length=2000 strand=+", "m64011_190830_220126/1/ccs", b"x" * 300, b"a\tb", "répétition", b"0"]
    ids = [kinds[int(i)] for i in rng.randint(0, len(kinds), size=n)]
    ids = [i + str(k).encode() if isinstance(i, bytes) and k % 3 == 0 and i else i for k, i in enumerate(ids)]
    return fields, read_len, units, ids


def fuzz_report(fields, units):
    """the Report of those rows, every row a read of its own, as numpy columns: the ratio column as mtr_report_device defines it"""
    n = len(fields)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = fields[:, 5].astype(np.float32) / fields[:, 2].astype(np.float32)
    bits = ratio.view(np.uint32).copy()
    bits[np.isnan(ratio)] = RATIO_NAN_BITS
    unit_off = np.zeros(n + 1, np.int64)
    unit_off[1:] = np.cumsum([len(u) for u in units])
    return mtr_amd.Report(np.ones(n, np.int32), np.arange(n, dtype=np.int32), np.zeros(n, np.int32), fields, bits.view(np.float32), unit_off,
                          np.frombuffer(b"".join(units), np.uint8))


def _snprintf_f(x) -> str:
    libc = C.CDLL(None)
    libc.snprintf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_double]
    libc.snprintf.restype = C.c_int
    buf = C.create_string_buffer(80)
    n = libc.snprintf(buf, 80, b"%f", C.c_double(float(x)))
    return buf.raw[:n].decode()


def test_the_oracle_prints_the_fuzz_rows_ratios_as_glibc_does():
    fields, _, units, _ = fuzz_rows()
    ratio = fuzz_report(fields, units).ratio
    assert len(ratio) >= 3000
    seen = set()
    for k, x in enumerate(ratio):
        got = mtr_amd._c_float_text(x)
        assert got == _snprintf_f(x), (k, fields[k, 5], fields[k, 2], got)
        seen.add(got)
    for k, (_, _, want) in enumerate(PINNED):
        assert mtr_amd._c_float_text(ratio[k]) == want, PINNED[k]
    assert {"inf", "-inf", "-nan", "-0.000000"} <= seen
    assert any(s.startswith("-") and s[1].isdigit() and float(s) < -1 for s in seen) and any(float(s) > 1 for s in seen if s[-1].isdigit())


def test_the_oracle_prints_the_fuzz_rows_integers_as_c_does():
    fields, read_len, units, ids = fuzz_rows(n=400)
    text = mtr_amd.format_report(ids, read_len, fuzz_report(fields, units))
    lines = text.split(b"\n")[:-1]
    assert len(lines) == 400
    libc = C.CDLL(None)
    for k, line in enumerate(lines):
        bid = ids[k].encode() if isinstance(ids[k], str) else ids[k]
        assert line.startswith(bid + b"\t") and line.endswith(b"\t" + units[k])
        cols = line[len(bid) + 1:len(line) - len(units[k]) - 1].split(b"\t")
        assert len(cols) == 11, (k, line)
        want = [int(read_len[k]), int(fields[k, 0]) + 1, int(fields[k, 1]) + 1] + [int(v) for v in fields[k, 2:6]] + [None] + [int(v) for v in fields[k, 6:9]]
        for c, w in zip(cols, want):
            if w is not None:
                buf = C.create_string_buffer(16)
                n = libc.snprintf(buf, 16, b"%d", C.c_int(w))
                assert c == buf.raw[:n], (k, c, w)
    flat = set(fields.ravel().tolist())
    assert {0, INT_MIN, INT_MAX} <= flat and any(v < 0 for v in flat)


def test_pack_ids():
    data, off = mtr_amd.pack_ids(["a", b"bc", "", bytearray(b"xyz"), "é"], 5)
    assert off.dtype == np.int64 and off.tolist() == [0, 1, 3, 3, 6, 8] and data.dtype == np.uint8
    assert data.tobytes()[:8] == b"abcxyz\xc3\xa9" and data.flags["C_CONTIGUOUS"] and len(data) >= 8
    data, off = mtr_amd.pack_ids([], 0)
    assert off.tolist() == [0] and len(data) >= 1                  # never a NULL pointer
    data, off = mtr_amd.pack_ids(["", ""])
    assert off.tolist() == [0, 0, 0] and len(data) >= 1
    with pytest.raises(mtr_amd.MtrError, match="2 ids for 3"):
        mtr_amd.pack_ids(["a", "b"], 3)
    with pytest.raises(mtr_amd.MtrError, match="id 1 must be str or bytes"):
        mtr_amd.pack_ids(["a", 7], 2)
    for bad in ("abc", b"abc", 5, None):
        with pytest.raises(mtr_amd.MtrError, match="sequence of str or bytes"):
            mtr_amd.pack_ids(bad, 3)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.mark.parametrize("method", ["report_text", "report_bytes"])
def test_a_wrong_id_count_raises_before_the_library_is_called(method):
    e = mtr_amd.Engine.__new__(mtr_amd.Engine)                     # no device: the checks come first
    e.lib, e.h, e.device, e.n_reads = _NoLibrary(), None, 0, 3
    for alignments in (False, True):
        with pytest.raises(mtr_amd.MtrError, match="2 ids for 3 uploaded reads"):
            getattr(e, method)(["a", "b"], alignments=alignments)
        with pytest.raises(mtr_amd.MtrError, match="id 2 must be str or bytes"):
            getattr(e, method)(["a", "b", 3.5], alignments=alignments)
    e.h = None


def test_the_entry_points_are_declared_and_exported():
    pub = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    tst = open(os.path.join(ROOT, "include", "mtr_hip_test.h")).read()
    assert re.search(r"mtr_status\s+mtr_report_text_device\(mtr_ctx \*ctx, const char \*ids, const int64_t \*id_off, int32_t with_alignments,\s*"
                     r"const mtr_report_text_dst \*dst, int64_t \*out_bytes\);", pub)
    m = re.search(r"typedef struct mtr_report_text_dst \{(.*?)\} mtr_report_text_dst;", pub, re.S)
    assert m and re.findall(r"(uint8_t|int64_t)\s*\*?\s*(\w+);", m.group(1)) == [("uint8_t", "text"), ("int64_t", "read_off"), ("int64_t", "cap_bytes")]
    assert "#define MTR_ABI_VERSION 5" in pub
    assert re.search(r"mtr_status\s+mtr_test_report_lines\(", tst) and "mtr_test_report_lines" not in pub
    assert {"mtr_report_text_device", "mtr_test_report_lines"} <= set(mtr_amd.EXPORTS)
    assert [f[0] for f in mtr_amd.CReportTextDst._fields_] == ["text", "read_off", "cap_bytes"] and C.sizeof(mtr_amd.CReportTextDst) == 24
    assert mtr_amd.ReportText._fields == ("text", "read_off")
    if os.path.exists(mtr_amd.LIB_PATH):
        lib = mtr_amd.load_library()
        for name in mtr_amd.EXPORTS:
            assert getattr(lib, name) is not None, name
        assert lib.mtr_report_text_device.argtypes is not None and lib.mtr_test_report_lines.argtypes is not None
