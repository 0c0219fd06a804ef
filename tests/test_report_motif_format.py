"""The motif catalogue (mtr_report_motifs_device, Engine.report_motif_tensors) without a device: format_motifs and MotifCatalog on hand-made
group tables, and the declarations - both headers, EXPORTS, the ctypes mirror of mtr_report_motif_dst, the built library's symbols."""
import ctypes as C
import os
import re

import numpy as np

import mtr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(rows, per_repeat=0):
    """a ReportMotifs of numpy columns from rows (motif, repeats, reads, copies, bases); the per-repeat columns are not what is printed"""
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r[0]) for r in rows])
    col = lambda i, dt: np.array([r[i] for r in rows], dt)        # noqa: E731
    z = np.zeros(per_repeat, np.int32)
    return mtr_amd.ReportMotifs(z.astype(np.uint8), z, z, z, off, np.frombuffer(b"".join(r[0] for r in rows), np.uint8),
                                np.arange(len(rows), dtype=np.int32), col(1, np.int32), col(2, np.int32), col(3, np.int64), col(4, np.int64))


A = [(b"AGC", 3, 2, 41, 130), (b"AC", 5, 5, 2 ** 33, 2 ** 34 + 1), (b"AAAAT", 1, 1, 7, 35)]
B = [(b"AATGG", 2, 2, 30, 151), (b"AC", 1, 1, 10, 20), (b"", 1, 1, 0, 12)]


def test_format_motifs_prints_one_line_per_group_in_group_order():
    assert mtr_amd.format_motifs(table(A)) == b"AGC\t3\t3\t2\t41\t130\nAC\t2\t5\t5\t8589934592\t17179869185\nAAAAT\t5\t1\t1\t7\t35\n"
    assert mtr_amd.format_motifs(table(B)).split(b"\n")[2] == b"\t0\t1\t1\t0\t12"          # the empty motif of a repeat without a unit
    assert mtr_amd.format_motifs(table([])) == b""


def test_a_catalog_adds_every_column_of_a_shared_motif_and_keeps_first_appearance_order():
    cat = mtr_amd.MotifCatalog()
    assert len(cat) == 0 and cat.rows() == [] and cat.format() == b""
    assert cat.add(table(A)) is cat
    assert cat.format() == mtr_amd.format_motifs(table(A))          # one batch: the batch's own table
    cat.add(table(B))
    assert cat.rows() == [(b"AGC", 3, 3, 2, 41, 130), (b"AC", 2, 6, 6, 2 ** 33 + 10, 2 ** 34 + 21), (b"AAAAT", 5, 1, 1, 7, 35),
                          (b"AATGG", 5, 2, 2, 30, 151), (b"", 0, 1, 1, 0, 12)]
    assert cat.format().split(b"\n")[1] == b"AC\t2\t6\t6\t8589934602\t17179869205" and len(cat) == 5
    other = mtr_amd.MotifCatalog().add(table(B)).add(table(A))      # the other order of batches: the same rows in another order
    assert sorted(other.rows()) == sorted(cat.rows()) and [r[0] for r in other.rows()] == [b"AATGG", b"AC", b"", b"AGC", b"AAAAT"]
    cat.add(table([]))
    assert len(cat) == 5


def test_the_entry_points_are_declared_and_exported():
    pub = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    tst = open(os.path.join(ROOT, "include", "mtr_hip_test.h")).read()
    assert re.search(r"mtr_status\s+mtr_report_motifs_device\(mtr_ctx \*ctx, const mtr_report_motif_dst \*dst,\s*"
                     r"int64_t \*out_repeats, int64_t \*out_groups, int64_t \*out_motif_bytes\);", pub)
    m = re.search(r"typedef struct mtr_report_motif_dst \{(.*?)\} mtr_report_motif_dst;", pub, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip().split(None, 1)[1] if decl.strip() else "")]
    want = ["strand", "rotation", "motif_len", "group", "motif_off", "motifs", "g_first", "g_repeats", "g_reads", "g_copies", "g_bases",
            "cap_repeats", "cap_groups", "cap_motif_bytes"]
    assert names == want, names
    assert "#define MTR_ABI_VERSION 5" in pub
    assert re.search(r"mtr_status\s+mtr_test_unit_motifs\(", tst) and "mtr_test_unit_motifs" not in pub
    assert {"mtr_report_motifs_device", "mtr_test_unit_motifs"} <= set(mtr_amd.EXPORTS)
    assert [f[0] for f in mtr_amd.CReportMotifDst._fields_] == want and C.sizeof(mtr_amd.CReportMotifDst) == 14 * 8
    assert mtr_amd.ReportMotifs._fields == tuple(want[:11])


def test_the_built_library_exports_them_and_keeps_its_abi():
    if not os.path.exists(mtr_amd.LIB_PATH):                        # as tests/test_report_resources.py: the code object needs no device
        from mtr_amd import build as mtr_build
        mtr_build.build()
    lib = mtr_amd.load_library()
    for name in mtr_amd.EXPORTS:
        assert getattr(lib, name) is not None, name
    assert len(lib.mtr_report_motifs_device.argtypes) == 5 and len(lib.mtr_test_unit_motifs.argtypes) == 20
    assert lib.mtr_abi_version() == 5
