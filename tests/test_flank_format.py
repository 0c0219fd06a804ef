"""mtr_amd.format_flank_hits and mtr_amd.format_genotypes on hand-made columns (CPU), and the declarations the two calls add to the public
header and to the ctypes mirror."""
import os
import re

import numpy as np
import pytest

import mtr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flank_hits():
    return mtr_amd.FlankHits(np.array([[0, 2], [1, 3]], np.int32), np.array([[3, 0], [1, 0]], np.int32), np.array([[6, 0], [4, 0]], np.int32),
                             np.array([[0, 0], [1, 0]], np.uint8))


def test_format_flank_hits():
    text = mtr_amd.format_flank_hits(["r0", b"r1"], [10, 20], ["ACG", b"TTC"], _flank_hits())
    assert text == (b"r0\t10\t0\t0\t0\t4\t6\t3\tACG\n" b"r0\t10\t1\t0\t2\t1\t0\t3\tTTC\n"
                    b"r1\t20\t0\t1\t1\t2\t4\t3\tCGT\n" b"r1\t20\t1\t0\t3\t1\t0\t3\tTTC\n")
    assert mtr_amd.format_flank_hits(["r0", "r1"], [10, 20], ["ACG", "TTC"], _flank_hits(), max_dist=1) == b"r0\t10\t0\t0\t0\t4\t6\t3\tACG\n" b"r1\t20\t0\t1\t1\t2\t4\t3\tCGT\n"
    assert mtr_amd.format_flank_hits(["r0", "r1"], [10, 20], ["ACG", "TTC"], _flank_hits(), max_dist=-1) == b""
    with pytest.raises(mtr_amd.MtrError, match="lengths"):
        mtr_amd.format_flank_hits(["r0", "r1"], [10], ["ACG", "TTC"], _flank_hits())


def _genotypes():
    z = lambda *s, t=np.int32: np.zeros(s, t)      # noqa: E731
    gt = mtr_amd.Genotypes(z(2, 2, t=np.uint8), z(2, 2, t=np.uint8), z(2, 2, 2), z(2, 2, 2), z(2, 2, 8), z(2, 2), z(2, 2, t=np.float32))
    # read 0, locus 1: orientation 1, ten copies of a three-base motif with one mismatch and one insertion; read 1, locus 0: an empty window
    gt.spanning[0, 1], gt.orientation[0, 1], gt.flank_dist[0, 1], gt.window[0, 1] = 1, 1, (2, 0), (40, 71)
    gt.fields[0, 1], gt.score[0, 1], gt.ratio[0, 1] = (40, 70, 31, 10, 29, 1, 1, 0), 27, np.float32(29) / np.float32(31)
    gt.spanning[1, 0], gt.flank_dist[1, 0], gt.window[1, 0] = 1, (0, 1), (25, 25)
    return gt


def test_format_genotypes():
    loci = [("ACGTAC", "AAG", "TTGACA"), (b"GGATCC", b"CAG", b"TCTAGA")]
    text = mtr_amd.format_genotypes(["r0", b"r1"], [100, 60], loci, _genotypes())
    assert text == (b"r0\t100\t1\t1\t2\t0\t41\t71\t31\t10\t29\t0.935484\t1\t1\t0\tCTG\n"
                    b"r1\t60\t0\t0\t0\t1\t26\t25\t0\t0\t0\t0.000000\t0\t0\t0\tAAG\n")
    assert len(text.split(b"\n")[0].split(b"\t")) == 16
    none = _genotypes()
    none.spanning[:] = 0
    assert mtr_amd.format_genotypes(["r0", "r1"], [100, 60], loci, none) == b""
    with pytest.raises(mtr_amd.MtrError, match="lengths"):
        mtr_amd.format_genotypes(["r0", "r1"], [100], loci, _genotypes())


def test_the_header_declares_the_two_calls_and_the_mirror_follows_it():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    for name, struct, cls in (("mtr_search_flanks_device", "mtr_flank_hits_dst", mtr_amd.CFlankHitsDst), ("mtr_genotype_loci_device", "mtr_genotypes_dst", mtr_amd.CGenotypesDst)):
        assert re.search(rf"mtr_status {name}\(mtr_ctx \*ctx", hdr) and name in mtr_amd.EXPORTS
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
        assert re.findall(r"\*?(\w+);", body) == [f[0] for f in cls._fields_]
    for word in ("d(e)", "the smallest e with d(e) = dist", "the largest s <= end", "orientation 1", "orientation 0 on a tie"):
        assert word in hdr, word
    assert mtr_amd.FlankHits._fields == ("dist", "start", "end", "strand")
    assert mtr_amd.Genotypes._fields == ("spanning", "orientation", "flank_dist", "window", "fields", "score", "ratio")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "MTR_TEST_FLANK_WORD" in readme and "search_flanks" in readme and "genotype_loci" in readme
