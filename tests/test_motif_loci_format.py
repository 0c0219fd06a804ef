"""mtr_amd.format_motif_loci on hand-made columns, and the locus search's place in the header and the built library (CPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IDS, LENS, MOTIFS = ["read/1", b"read 2"], [140, 97], ["CAG", b"GGGGCC", "AT"]
# per pair (read, motif), in ascending start: (eight fields, score, ratio, strand)
ROWS = {(0, 0): [((2, 31, 30, 10, 29, 1, 0, 0), 28, 29 / 30, 0), ((40, 69, 30, 10, 30, 0, 0, 0), 30, 1.0, 1), ((100, 111, 12, 4, 12, 0, 0, 0), 12, 1.0, 0)],
        (0, 1): [((5, 16, 12, 2, 11, 0, 1, 0), 10, 11 / 12, 1)],
        (1, 0): [((0, 96, 97, 31, 90, 3, 4, 2), 81, 90 / 97, 1)],
        (1, 2): [((10, 13, 4, 2, 4, 0, 0, 0), 4, 1.0, 0), ((20, 25, 6, 3, 6, 0, 0, 0), 6, 1.0, 0)]}


def _loci(rows, n, m):
    off, f, s, r, st = [0], [], [], [], []
    for p in range(n * m):
        for fields, score, ratio, strand in rows.get(divmod(p, m), []):
            f.append(fields); s.append(score); r.append(ratio); st.append(strand)
        off.append(len(f))
    return mtr_amd.MotifLoci(np.array(off, np.int64), np.array(f, np.int32).reshape(-1, 8), np.array(s, np.int32), np.array(r, np.float32),
                             np.array(st, np.uint8), np.zeros((n, m), np.uint8))


def test_the_thirteen_columns_ordered_by_read_motif_start():
    lines = mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, _loci(ROWS, 2, 3)).split(b"\n")
    assert lines[-1] == b"" and len(lines) == 8
    assert lines[0] == b"read/1\t140\t3\t32\t30\t3\t10\t29\t0.966667\t1\t0\t0\tCAG"
    assert lines[1] == b"read/1\t140\t41\t70\t30\t3\t10\t30\t1.000000\t0\t0\t0\tCTG"            # strand 1: the reverse complement, as aligned
    assert lines[2] == b"read/1\t140\t101\t112\t12\t3\t4\t12\t1.000000\t0\t0\t0\tCAG"
    assert lines[3] == b"read/1\t140\t6\t17\t12\t6\t2\t11\t0.916667\t0\t1\t0\tGGCCCC"
    assert lines[4] == b"read 2\t97\t1\t97\t97\t3\t31\t90\t0.927835\t3\t4\t2\tCTG"
    assert lines[5] == b"read 2\t97\t11\t14\t4\t2\t2\t4\t1.000000\t0\t0\t0\tAT"
    assert lines[6] == b"read 2\t97\t21\t26\t6\t2\t3\t6\t1.000000\t0\t0\t0\tAT"
    assert all(len(ln.split(b"\t")) == 13 for ln in lines[:-1])


def test_a_single_locus_prints_as_format_motif_hits_prints_the_hit():
    fields, score, ratio, strand = ROWS[(1, 0)][0]
    hits = mtr_amd.MotifHits(np.array([[fields]], np.int32), np.array([[score]], np.int32), np.array([[ratio]], np.float32), np.array([[strand]], np.uint8))
    assert mtr_amd.format_motif_loci(["r"], [97], ["CAG"], _loci({(0, 0): ROWS[(1, 0)]}, 1, 1)) == mtr_amd.format_motif_hits(["r"], [97], ["CAG"], hits)


def test_the_filters_filter_and_an_empty_pair_prints_nothing():
    loci = _loci(ROWS, 2, 3)
    by_ratio = mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, loci, min_ratio=0.95).split(b"\n")[:-1]
    assert [ln.split(b"\t")[8] for ln in by_ratio] == [b"0.966667", b"1.000000", b"1.000000", b"1.000000", b"1.000000"]
    by_copies = mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, loci, min_copies=4).split(b"\n")[:-1]
    assert [ln.split(b"\t")[6] for ln in by_copies] == [b"10", b"10", b"4", b"31"]
    assert mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, loci, min_ratio=0.99, min_copies=11) == b""
    assert mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, _loci({}, 2, 3)) == b""
    only = mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, _loci({(1, 2): ROWS[(1, 2)]}, 2, 3)).split(b"\n")[:-1]       # five empty pairs before it
    assert len(only) == 2 and all(ln.startswith(b"read 2\t") and ln.endswith(b"\tAT") for ln in only)


def test_length_mismatches_raise():
    loci = _loci(ROWS, 2, 3)
    with pytest.raises(mtr_amd.MtrError, match="lengths"):
        mtr_amd.format_motif_loci(IDS, LENS[:1], MOTIFS, loci)
    with pytest.raises(mtr_amd.MtrError, match="offsets"):
        mtr_amd.format_motif_loci(IDS, LENS, MOTIFS[:2], loci)
    with pytest.raises(mtr_amd.MtrError, match="offsets"):
        mtr_amd.format_motif_loci(IDS + ["r3"], LENS + [5], MOTIFS, loci)
    with pytest.raises(mtr_amd.MtrError, match="rows"):
        mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, loci._replace(score=loci.score[:-1]))
    with pytest.raises(mtr_amd.MtrError, match="rows"):
        mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, loci._replace(fields=loci.fields[:-2]))
    with pytest.raises(mtr_amd.MtrError, match="ascend"):
        off = loci.loci_off.copy(); off[1], off[2] = off[2], off[1] - 1
        mtr_amd.format_motif_loci(IDS, LENS, MOTIFS, loci._replace(loci_off=off))


def test_the_header_declares_the_entry_points_and_still_says_abi_5():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+5\b", hdr)
    assert re.search(r"mtr_status\s+mtr_search_motif_loci_device\s*\(\s*mtr_ctx\s*\*ctx,\s*const char\s*\*motifs,\s*const int64_t\s*\*motif_off,\s*int32_t n_motifs", hdr)
    assert re.search(r"mtr_status\s+mtr_motif_loci_copy_device\s*\(\s*mtr_ctx\s*\*ctx,\s*const mtr_motif_loci_dst\s*\*dst\)", hdr)
    assert "typedef struct mtr_motif_loci_dst" in hdr and "cap_pairs, cap_loci" in hdr


def test_the_built_library_exports_the_symbols():
    assert {"mtr_search_motif_loci_device", "mtr_motif_loci_copy_device"} <= set(mtr_amd.EXPORTS)
    lib = mtr_amd.load_library()
    assert lib.mtr_abi_version() == 5
    assert isinstance(lib.mtr_search_motif_loci_device, C._CFuncPtr) and isinstance(lib.mtr_motif_loci_copy_device, C._CFuncPtr)
    assert [f[0] for f in mtr_amd.CMotifLociDst._fields_] == ["loci_off", "fields", "score", "ratio", "strand", "open", "cap_pairs", "cap_loci"]
    assert C.sizeof(mtr_amd.CMotifLociDst) == 64
