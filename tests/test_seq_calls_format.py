"""The sequence allele calls' declarations and text (CPU): the header declares the entry points and their limits, EXPORTS names them, the ctypes
mirrors of mtr_seq_params and mtr_seq_calls_dst have the header's fields in its order - the first eight of the latter are mtr_allele_calls_dst's -
the source list of the build has the new files, README names the test switch, and format_sequence_calls prints hand-made columns as literal
lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd
import mtr_amd.build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(hdr, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", hdr, re.S).group(1)
    return re.findall(r"^\s*(?:int64_t|int32_t|uint8_t)\s*\*?\s*(\w+);", body, re.M)


def test_the_header_exports_and_the_ctypes_mirrors():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    for name in ("mtr_call_alleles_sequence_device", "mtr_call_alleles_sequence_copy_device"):
        assert re.search(rf"mtr_status {name}\(mtr_ctx \*ctx", hdr) and name in mtr_amd.EXPORTS, name
    assert "#define MTR_ABI_VERSION 5" in hdr and "#define MTR_SEQ_MAX_DIST 254" in hdr and "#define MTR_SEQ_MAX_MEMBERS 128" in hdr
    assert (mtr_amd.SEQ_MAX_DIST, mtr_amd.SEQ_MAX_MEMBERS) == (254, 128)
    assert _fields(hdr, "mtr_seq_params") == [f for f, _ in mtr_amd.CSeqParams._fields_] == ["max_dist", "min_support", "min_percent", "min_sep", "min_gain"]
    dst = [f for f, _ in mtr_amd.CSeqCallsDst._fields_]
    assert _fields(hdr, "mtr_seq_calls_dst") == dst and C.sizeof(mtr_amd.CSeqCallsDst) == 16 * 8 and C.sizeof(mtr_amd.CSeqParams) == 20
    assert dst[:8] == _fields(hdr, "mtr_allele_calls_dst")[:8] == list(mtr_amd.AlleleCalls._fields)
    assert dst[8:] == list(mtr_amd.SequenceCalls._fields[1:]) + ["cap_loci", "cap_support", "cap_pairs"]
    assert {"seq_calls.hip.inc", "seq_calls.h"} <= set(mtr_amd.build.SOURCES)
    assert "MTR_TEST_SEQ_ROWS" in open(os.path.join(ROOT, "README.md")).read()


def _calls():
    i32, i64, u8 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.int64)), (lambda *v: np.array(v, np.uint8))
    ac = mtr_amd.AlleleCalls(i64(0, 5, 5, 8, 10), i32(20, 20, 20, 20, 20, 7, 7, 7, 3, 3), i32(0, 2, 4, 1, 3, 5, 6, 9, 1, 2), u8(0, 0, 0, 1, 1, 0, 0, 0, 0, 0),
                             u8(2, 0, 1, 0), i32(20, 20, 0, 0, 7, 7, 0, 0).reshape(4, 2), i32(3, 2, 0, 0, 3, 0, 0, 0).reshape(4, 2), i64(31, 4, 0, 0, 5, 5, 0, 0).reshape(4, 2))
    return mtr_amd.SequenceCalls(ac, i32(2, 3, -1, -1, 6, -1, -1, -1).reshape(4, 2), i32(1, 0, 2, 0, 1, 2, 0, 3, 0, 0), u8(0, 0, 0, 1), i64(0, 10, 10, 13, 13), np.zeros(13, np.uint8))


def test_the_text_of_hand_made_columns():
    loci = [("A", "CAG", "C"), ("A", "GAA", "C"), ("A", "CGG", "C"), ("A", "T", "C")]
    text = mtr_amd.format_sequence_calls(loci, _calls())
    assert text == (b"0\t5\t2\t20\t20\t3\t2\t31\t4\t20\t20\tCAG\t2\t3/3\t3\t1/2\n"
                    b"1\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\tGAA\t-1\t0/0\t-1\t0/0\n"
                    b"2\t3\t1\t7\t7\t3\t0\t5\t5\t7\t7\tCGG\t6\t5/3\t-1\t0/0\n"
                    b"3\t2\t0\t0\t0\t0\t0\t0\t0\t3\t3\tT\t-1\t0/0\t-1\t0/0\n")
    plain = mtr_amd.format_allele_calls(loci, _calls().calls).splitlines()
    assert [line.startswith(p + b"\t") for line, p in zip(text.splitlines(), plain)] == [True] * 4


def test_mismatched_columns_are_refused():
    sc = _calls()
    with pytest.raises(mtr_amd.MtrError, match="3 medoid pairs for 4 loci"):
        mtr_amd.format_sequence_calls([("A", "CAG", "C")] * 4, sc._replace(medoid=sc.medoid[:3]))
