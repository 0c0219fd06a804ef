"""The window edits' declarations and text (CPU): the header declares the entry points and what they need, EXPORTS names them, the ctypes mirror of
mtr_window_edits_dst has the header's fields in its order, the source list of the build has the new files, and format_window_edits prints the
reference's edits as literal lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd
import mtr_amd.build
from tests import window_edits_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_exports_and_the_ctypes_mirror():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    test_hdr = open(os.path.join(ROOT, "include", "mtr_hip_test.h")).read()
    for name in ("mtr_window_edits_device", "mtr_window_edits_copy_device"):
        assert re.search(rf"mtr_status {name}\(mtr_ctx \*ctx", hdr) and name in mtr_amd.EXPORTS, name
    assert "mtr_status mtr_test_window_edits_rounds(mtr_ctx *ctx" in test_hdr and "mtr_test_window_edits_rounds" in mtr_amd.EXPORTS
    assert "#define MTR_ABI_VERSION 5" in hdr and "#define MTR_WE_FIELDS 6" in hdr and "#define MTR_WE_SCRATCH_BYTES" in hdr and mtr_amd.WE_FIELDS == 6
    body = re.search(r"typedef struct mtr_window_edits_dst \{(.*?)\} mtr_window_edits_dst;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(?:int64_t|int32_t|uint8_t)\s*\*?\s*(\w+);", body, re.M)
    assert fields == [f for f, _ in mtr_amd.CWindowEditsDst._fields_] == ["off", "edits", "seg", "score", "skipped", "cap_windows", "cap_edits"]
    assert C.sizeof(mtr_amd.CWindowEditsDst) == 7 * 8
    assert mtr_amd.WindowEdits._fields == ("off", "edits", "seg", "score", "skipped")
    assert {"window_edits.hip.inc", "window_edits.h"} <= set(mtr_amd.build.SOURCES)
    assert "MTR_TEST_WE_SCRATCH_BYTES" in open(os.path.join(ROOT, "README.md")).read()


def _we(structures, windows, which):
    off, edits, seg, score, skipped = ref.columns(structures, windows, which)
    return mtr_amd.WindowEdits(off, edits, seg, score, skipped)


def test_the_text_of_hand_worked_windows():
    structures = [["CAG"], ["CAG", "CCG"]]
    windows = ["CAG" * 10 + "CAA" + "CAG" * 9, "CAGCAG" + "CATG" + "CAG", "CAGCAG" + "AG" + "CAG", "CAGCAG" + "CCG" + "CTG" + "CCG", "TT", ""]
    which = [0, 0, 0, 1, 1, 0]
    we = _we(structures, windows, which)
    text = mtr_amd.format_window_edits([structures[k] for k in which], we, names=["htt", "ins", "del", "two", "none", "empty"])
    assert text == (b"htt\t1\tCAG#10:2G>A@32\n"
                    b"ins\t1\tCAG#2:1+T@8\n"
                    b"del\t1\tCAG#2:0-C@6\n"
                    b"two\t1\tCCG#1:1C>T@10\n"
                    b"none\t0\n"
                    b"empty\t0\n")


def test_indices_as_names_one_structure_for_all_and_a_skipped_window():
    we = _we([["CAG"]], ["CTGCAGCAA", np.zeros(ref.MAX_WINDOW + 1, np.uint8)], [0, 0])
    assert mtr_amd.format_window_edits(["CAG"], we) == b"0\t2\tCAG#0:1A>T@1\tCAG#2:2G>A@8\n1\t0\tskipped\n"
    with pytest.raises(mtr_amd.MtrError, match="3 structures for 2 windows"):
        mtr_amd.format_window_edits(["CAG"] * 3, we)
