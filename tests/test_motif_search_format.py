"""mtr_amd.format_motif_hits on hand-made columns, and the known-motif search's place in the header and the built library (CPU)."""
import ctypes as C
import os
import re

import numpy as np

import mtr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hits(rows, n, m):
    """rows: {(read, motif): (eight fields, score, ratio, strand)}; every other hit is the no-hit value"""
    f = np.tile(np.array([0, -1, 0, 0, 0, 0, 0, 0], np.int32), (n, m, 1))
    s, r, st = np.zeros((n, m), np.int32), np.zeros((n, m), np.float32), np.zeros((n, m), np.uint8)
    for (i, j), (fields, score, ratio, strand) in rows.items():
        f[i, j], s[i, j], r[i, j], st[i, j] = fields, score, np.float32(ratio), strand
    return mtr_amd.MotifHits(f, s, r, st)


IDS, LENS, MOTIFS = ["read/1", b"read 2", "r3"], [40, 97, 12], ["CAG", b"GGGGCC", "AT"]
ROWS = {(0, 0): ((2, 31, 30, 10, 29, 1, 0, 0), 28, 29 / 30, 0),
        (0, 1): ((5, 16, 12, 2, 11, 0, 1, 0), 10, 11 / 12, 1),
        (1, 0): ((0, 96, 97, 31, 90, 3, 4, 2), 81, 90 / 97, 1),
        (1, 2): ((10, 13, 4, 2, 4, 0, 0, 0), 4, 1.0, 0),
        (2, 1): ((0, 5, 6, 1, 4, 2, 0, 0), 2, 4 / 6, 0)}


def test_the_thirteen_columns_in_read_then_motif_order():
    text = mtr_amd.format_motif_hits(IDS, LENS, MOTIFS, _hits(ROWS, 3, 3))
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) == 6
    assert lines[0] == b"read/1\t40\t3\t32\t30\t3\t10\t29\t0.966667\t1\t0\t0\tCAG"
    assert lines[1] == b"read/1\t40\t6\t17\t12\t6\t2\t11\t0.916667\t0\t1\t0\tGGCCCC"          # strand 1: the reverse complement, as aligned
    assert lines[2] == b"read 2\t97\t1\t97\t97\t3\t31\t90\t0.927835\t3\t4\t2\tCTG"
    assert lines[3] == b"read 2\t97\t11\t14\t4\t2\t2\t4\t1.000000\t0\t0\t0\tAT"
    assert lines[4] == b"r3\t12\t1\t6\t6\t6\t1\t4\t0.666667\t2\t0\t0\tGGGGCC"
    assert all(len(ln.split(b"\t")) == 13 for ln in lines[:-1])


def test_score_zero_is_never_printed_and_the_filters_filter():
    rows = dict(ROWS)
    rows[(2, 0)] = ((0, -1, 0, 0, 0, 0, 0, 0), 0, 0.0, 0)
    rows[(2, 2)] = ((3, 4, 2, 1, 2, 0, 0, 0), 0, 1.0, 0)                     # (no search returns this: score 0 alone decides)
    hits = _hits(rows, 3, 3)
    assert mtr_amd.format_motif_hits(IDS, LENS, MOTIFS, hits) == mtr_amd.format_motif_hits(IDS, LENS, MOTIFS, _hits(ROWS, 3, 3))
    by_ratio = mtr_amd.format_motif_hits(IDS, LENS, MOTIFS, hits, min_ratio=0.92).split(b"\n")[:-1]
    assert [ln.split(b"\t")[8] for ln in by_ratio] == [b"0.966667", b"0.927835", b"1.000000"]
    by_copies = mtr_amd.format_motif_hits(IDS, LENS, MOTIFS, hits, min_copies=3).split(b"\n")[:-1]
    assert [ln.split(b"\t")[6] for ln in by_copies] == [b"10", b"31"]
    assert mtr_amd.format_motif_hits(IDS, LENS, MOTIFS, hits, min_ratio=0.95, min_copies=11) == b""
    empty = _hits({}, 3, 3)
    assert mtr_amd.format_motif_hits(IDS, LENS, MOTIFS, empty) == b""


def test_the_ratio_prints_as_format_report_prints_the_same_float():
    for mat, ln in ((29, 30), (1, 3), (2, 3), (90, 97), (1, 7), (499, 500), (5, 5)):
        ratio = np.float32(mat) / np.float32(ln)
        hits = _hits({(0, 0): ((0, ln - 1, ln, 1, mat, ln - mat, 0, 0), 1, ratio, 0)}, 1, 1)
        line = mtr_amd.format_motif_hits(["r"], [ln], ["CAG"], hits)
        rep = mtr_amd.Report(np.ones(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.array([[0, ln - 1, ln, 3, 1, mat, ln - mat, 0, 0, 0, 1, 1, 1, 0]], np.int32),
                             np.array([ratio], np.float32), np.array([0, 3], np.int64), np.frombuffer(b"CAG", np.uint8))
        want = mtr_amd.format_report(["r"], [ln], rep)
        assert line == want, (line, want)


def test_the_header_declares_the_entry_point_and_still_says_abi_5():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+5\b", hdr)
    assert re.search(r"mtr_status\s+mtr_search_motifs_device\s*\(\s*mtr_ctx\s*\*ctx,\s*const char\s*\*motifs,\s*const int64_t\s*\*motif_off,\s*int32_t n_motifs", hdr)
    assert "typedef struct mtr_motif_hits_dst" in hdr and "cap_hits" in hdr
    test_hdr = open(os.path.join(ROOT, "include", "mtr_hip_test.h")).read()
    assert "MTR_TEST_MOTIF_LANE_MAX" in test_hdr and "MTR_TEST_MOTIF_LANE_ROWS" in test_hdr


def test_the_built_library_exports_the_symbol():
    assert "mtr_search_motifs_device" in mtr_amd.EXPORTS
    lib = mtr_amd.load_library()
    assert lib.mtr_abi_version() == 5
    assert isinstance(lib.mtr_search_motifs_device, C._CFuncPtr)
    assert [f[0] for f in mtr_amd.CMotifHitsDst._fields_] == ["fields", "score", "ratio", "strand", "cap_hits"]
    assert C.sizeof(mtr_amd.CMotifHitsDst) == 40
