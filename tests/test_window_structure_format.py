"""The window structure's declarations and text (CPU): the header declares the entry point and its limits, EXPORTS names it, the ctypes mirror of
mtr_window_structure_dst has the header's fields in the header's order, and format_window_structure / with_segment_copies over plain arrays."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import mtr_amd
from tests import window_structure_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_the_exports_and_the_mirror_agree():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    assert re.search(r"mtr_status mtr_window_structure_device\(mtr_ctx \*ctx", hdr) and "mtr_window_structure_device" in mtr_amd.EXPORTS
    assert f"#define MTR_WS_MAX_SEGMENTS {mtr_amd.WS_MAX_SEGMENTS}" in hdr and f"#define MTR_WS_MAX_WINDOW {mtr_amd.WS_MAX_WINDOW}" in hdr and "#define MTR_ABI_VERSION 5" in hdr
    assert (mtr_amd.WS_MAX_SEGMENTS, mtr_amd.WS_MAX_WINDOW) == (ref.MAX_SEGMENTS, ref.MAX_WINDOW)
    body = re.search(r"typedef struct mtr_window_structure_dst \{(.*?)\} mtr_window_structure_dst;", hdr, re.S).group(1)
    assert re.findall(r"\*?(\w+);", body) == [f[0] for f in mtr_amd.CWindowStructureDst._fields_] == ["seg", "score", "ratio", "skipped", "cap_windows"]
    src = open(os.path.join(ROOT, "mtr_amd", "csrc", "window_structure.h")).read()
    assert "#define WS_MAX_SEGMENTS 4" in src and "#define WS_MAX_WINDOW 16384" in src


def test_the_text_of_a_result():
    structures = [["CAG", "CAA", "CAG"], "GAA", ["A"]]
    windows = ["CAG" * 10 + "CAA" + "CAG" * 9, "", "A"]
    seg, score, ratio, skipped = ref.columns(structures, windows, [0, 1, 2])
    skipped[2] = 1
    ws = mtr_amd.WindowStructure(seg, score, ratio, skipped)
    assert mtr_amd.format_window_structure(structures, ws, names=["x", "y", "z"]) == \
        b"x\t60\t1.0000\tCAG*10[0,30)30\tCAA*1[30,33)3\tCAG*9[33,60)27\ny\t0\t0.0000\tGAA*0[0,0)0\nz\t1\t1.0000\tskipped\n"
    assert mtr_amd.format_window_structure(["GAA"], ws).splitlines()[1] == b"1\t0\t0.0000\tGAA*0[0,0)0"
    with pytest.raises(mtr_amd.MtrError, match="2 structures for 3 windows"):
        mtr_amd.format_window_structure(structures[:2], ws)


def test_with_segment_copies_refuses_what_does_not_fit():
    sg = SimpleNamespace(read=np.zeros(3, np.int32))
    ws = mtr_amd.WindowStructure(np.zeros((2, 4, 4), np.int32), None, None, None)
    with pytest.raises(mtr_amd.MtrError, match="segment must be an integer in 0..3"):
        mtr_amd.with_segment_copies(sg, ws, 4)
    with pytest.raises(mtr_amd.MtrError, match=r"\(2, 4, 4\) segment columns for 3 rows"):
        mtr_amd.with_segment_copies(sg, ws, 0)
