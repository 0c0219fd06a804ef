"""mtr_amd.format_allele_calls on hand-made columns and mtr_amd.genotype_rows_args on wrong inputs (CPU), and the declarations the call adds to
the public header and to the ctypes mirror."""
import os
import re

import numpy as np
import pytest

import mtr_amd

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _calls():
    # locus 0: 20 x 6 and 35 x 5 with stutter; locus 1: no support; locus 2: one allele of three reads
    value = [19, 20, 20, 20, 20, 21, 34, 35, 35, 35, 36, 7, 7, 8]
    return mtr_amd.AlleleCalls(np.array([0, 11, 11, 14], np.int64), np.array(value, np.int32), np.arange(14, dtype=np.int32), np.array([0] * 6 + [1] * 5 + [0] * 3, np.uint8),
                               np.array([2, 0, 1], np.uint8), np.array([[20, 35], [0, 0], [7, 7]], np.int32), np.array([[6, 5], [0, 0], [3, 0]], np.int32),
                               np.array([[76, 4], [0, 0], [2 ** 31 + 1, 2 ** 31 + 1]], np.int64))


def test_format_allele_calls():
    loci = [("ACGTAC", "CAG", "TTGACA"), (b"GGATCC", b"TTC", b"TCTAGA"), ("AAAC", "GGCCTA", "CCCA")]
    text = mtr_amd.format_allele_calls(loci, _calls())
    assert text == (b"0\t11\t2\t20\t35\t6\t5\t76\t4\t19\t36\tCAG\n" b"1\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\tTTC\n"
                    b"2\t3\t1\t7\t7\t3\t0\t2147483649\t2147483649\t7\t8\tGGCCTA\n")
    assert all(len(line.split(b"\t")) == 12 for line in text.splitlines())
    assert mtr_amd.format_allele_calls(loci, mtr_amd.AlleleCalls(*[torch.from_numpy(c) for c in _calls()])) == text
    with pytest.raises(mtr_amd.MtrError, match="loci"):
        mtr_amd.format_allele_calls(loci[:2], _calls())


def _rows(n=3, m=2):
    z = lambda dtype, *tail: torch.zeros((n, m) + tail, dtype=dtype)      # noqa: E731
    return mtr_amd.Genotypes(z(torch.uint8), z(torch.uint8), z(torch.int32, 2), z(torch.int32, 2), z(torch.int32, 8), z(torch.int32), z(torch.float32))


def test_genotype_rows_args_refuses():
    good = _rows()
    bad = [
        (good._replace(spanning=good.spanning.numpy()), "spanning must be a torch.Tensor"),
        (good._replace(spanning=good.spanning.to(torch.int32)), "spanning must have dtype torch.uint8"),
        (good._replace(spanning=good.spanning.reshape(-1)), r"spanning must be \[n, m\]"),
        (good._replace(spanning=torch.zeros((0, 2), dtype=torch.uint8)), r"spanning must be \[n, m\]"),
        (good._replace(spanning=torch.zeros((3, 0), dtype=torch.uint8)), r"spanning must be \[n, m\]"),
        (good._replace(spanning=torch.zeros((2, 3), dtype=torch.uint8).t()), "spanning must be contiguous"),
        (good._replace(window=None), "window must be a torch.Tensor"),
        (good._replace(window=good.window.to(torch.int64)), "window must have dtype torch.int32"),
        (good._replace(window=good.window[:, :, :1].contiguous()), "window must have shape"),
        (good._replace(window=torch.zeros((3, 2, 4), dtype=torch.int32)[:, :, ::2]), "window must be contiguous"),
        (good._replace(fields=good.fields.to(torch.float32)), "fields must have dtype torch.int32"),
        (good._replace(fields=torch.zeros((3, 2, 7), dtype=torch.int32)), "fields must have shape"),
        (good._replace(fields=torch.zeros((2, 3, 8), dtype=torch.int32).transpose(0, 1)), "fields must be contiguous"),
        (good._replace(ratio=good.ratio.to(torch.float64)), "ratio must have dtype torch.float32"),
        (good._replace(ratio=torch.zeros((2, 2), dtype=torch.float32)), "ratio must have shape"),
        (good._replace(ratio=torch.zeros((2, 3), dtype=torch.float32).t()), "ratio must be contiguous"),
        (good, "must be GPU tensors"),                        # everything else in order: a CPU tensor is refused last
    ]
    for gt, why in bad:
        with pytest.raises(mtr_amd.MtrError, match=why):
            mtr_amd.genotype_rows_args(gt, 0)
    # the unread columns are not looked at
    with pytest.raises(mtr_amd.MtrError, match="must be GPU tensors"):
        mtr_amd.genotype_rows_args(good._replace(orientation=None, flank_dist=None, score="x"), 0)


def test_the_header_declares_the_call_and_the_mirror_follows_it():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    assert re.search(r"mtr_status mtr_call_alleles_device\(mtr_ctx \*ctx", hdr) and "mtr_call_alleles_device" in mtr_amd.EXPORTS
    for struct, cls in (("mtr_allele_params", mtr_amd.CAlleleParams), ("mtr_allele_calls_dst", mtr_amd.CAlleleCallsDst)):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
        assert re.findall(r"\*?(\w+);", body) == [f[0] for f in cls._fields_]
    for word in ("spanning == 1 and (window[1] == window[0] or ratio >= min_ratio)", "sorted by (v, read) ascending", "med(i, j) = v[i + (j - i - 1) / 2]",
                 "v[k - 1] < v[k]", "min(k, S_l - k) * 100 >= min_percent * S_l", "med(k, S_l) - med(0, k) >= min_sep", "the smallest such k on a tie",
                 "#define MTR_ALLELE_COPIES 0", "#define MTR_ALLELE_BASES 1", "#define MTR_ABI_VERSION 5"):
        assert word in hdr, word
    assert mtr_amd.AlleleCalls._fields == ("support_off", "value", "read", "allele", "zygosity", "call", "call_support", "cost")
    assert (mtr_amd.ALLELE_COPIES, mtr_amd.ALLELE_BASES) == (0, 1)
    assert [f[1] for f in mtr_amd.CAlleleParams._fields_] == [mtr_amd.C.c_int32, mtr_amd.C.c_float] + [mtr_amd.C.c_int32] * 3
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "call_alleles" in readme and "format_allele_calls" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7i-6" in design and "mtr_k_allele_rank" in design
