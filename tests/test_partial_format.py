"""format_partial_genotypes and partial_support (mtr_amd/__init__.py) on hand-made CPU tensors, and the declarations of the partial genotype:
the header, EXPORTS, the ctypes mirror of mtr_partial_dst."""
import os
import re

import pytest

import mtr_amd

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pg():
    """three reads, two loci"""
    t = lambda v, dt: torch.tensor(v, dtype=dt)      # noqa: E731
    partial = t([[1, 0], [1, 1], [0, 1]], torch.uint8)
    slot = t([[0, 0], [2, 1], [0, 3]], torch.uint8)
    fdist = t([[0, 0], [2, 1], [0, 3]], torch.int32)
    window = t([[[20, 60], [0, 0]], [[0, 30], [0, 45]], [[0, 0], [50, 50]]], torch.int32)
    ext = t([[[40, 41, 13, 38, 35, 0], [0] * 6], [[24, 24, 8, 24, 24, 6], [30, 28, 7, 27, 20, 15]], [[0] * 6, [0] * 6]], torch.int32)
    ratio = t([[0.95, 0.0], [1.0, 0.9], [0.0, 0.0]], torch.float32)
    is_open = t([[1, 0], [1, 0], [0, 1]], torch.uint8)
    return mtr_amd.PartialGenotypes(partial, slot, fdist, window, ext, ratio, is_open)


LOCI = [("ACGTACGTAC", "CAG", "TTGACCGATA"), (b"GGATCCAAGT", b"AAAG", b"CCATGGTTAA")]


def test_one_line_per_partial_row_and_open_rows_say_at_least():
    text = mtr_amd.format_partial_genotypes(["r0", b"r1", "r2"], [60, 70, 50], LOCI, _pg())
    assert text == (b"r0\t60\t0\t0\t0\t21\t60\t40\t>=13\t38\t0.950000\t35\t0\tCAG\n"
                    b"r1\t70\t0\t2\t2\t7\t30\t24\t>=8\t24\t1.000000\t24\t6\tCTG\n"
                    b"r1\t70\t1\t1\t1\t16\t45\t30\t7\t27\t0.900000\t20\t15\tAAAG\n"
                    b"r2\t50\t1\t3\t3\t51\t50\t0\t>=0\t0\t0.000000\t0\t0\tCTTT\n")
    as_numpy = mtr_amd.PartialGenotypes(*[c.numpy() for c in _pg()])
    assert mtr_amd.format_partial_genotypes(["r0", "r1", "r2"], [60, 70, 50], LOCI, as_numpy) == text
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.format_partial_genotypes(["r0", "r1", "r2"], [60, 70], LOCI, _pg())


def _calls(larger):
    z = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt)      # noqa: E731
    call = torch.tensor([[5, larger[0]], [7, larger[1]]], dtype=torch.int32)
    return mtr_amd.AlleleCalls(z(3, dt=torch.int64), z(0), z(0), z(0, dt=torch.uint8), torch.tensor([2, 1], dtype=torch.uint8), call, z(2, 2), z(2, 2, dt=torch.int64))


def test_partial_support_counts_and_n_beyond():
    s = mtr_amd.partial_support(_pg())
    assert s.n_partial.tolist() == [2, 2] and s.n_open.tolist() == [2, 1] and s.max_copies.tolist() == [13, 0] and s.n_beyond is None
    # the open rows of locus 0 hold 13 and 8 copies: against a larger called allele of 8 one row is beyond it, against 7 both, against 13 none
    assert mtr_amd.partial_support(_pg(), _calls((8, 7))).n_beyond.tolist() == [1, 0]
    assert mtr_amd.partial_support(_pg(), _calls((7, 0))).n_beyond.tolist() == [2, 0]
    assert mtr_amd.partial_support(_pg(), _calls((13, -1))).n_beyond.tolist() == [0, 1]           # (0 copies of an open row exceed -1)
    # min_ratio drops the row of ratio 0.95: the bound and the count fall to the other row's
    s = mtr_amd.partial_support(_pg(), _calls((7, 7)), min_ratio=0.96)
    assert s.max_copies.tolist() == [8, 0] and s.n_beyond.tolist() == [1, 0] and s.n_open.tolist() == [2, 1]
    # a closed row never counts, whatever its copies (locus 1's row of r1 holds 7)
    assert mtr_amd.partial_support(_pg(), _calls((0, 0))).n_beyond.tolist() == [2, 0]
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.partial_support(_pg(), mtr_amd.AlleleCalls(*[c[:1] if c.dim() == 2 else c for c in _calls((1, 1))]))
    empty = mtr_amd.PartialGenotypes(*[c[:0] for c in _pg()])
    assert mtr_amd.partial_support(empty).max_copies.tolist() == [0, 0] and mtr_amd.partial_support(empty).n_partial.tolist() == [0, 0]


def test_the_declarations_agree():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    assert re.search(r"mtr_status mtr_genotype_partial_device\(mtr_ctx \*ctx", hdr) and "mtr_genotype_partial_device" in mtr_amd.EXPORTS
    body = re.search(r"typedef struct mtr_partial_dst \{(.*?)\} mtr_partial_dst;", hdr, re.S).group(1)
    names = re.findall(r"\*?(\w+);", body)
    assert names == [f[0] for f in mtr_amd.CPartialDst._fields_], names
    assert [f[0] for f in mtr_amd.CPartialDst._fields_][:-1] == list(mtr_amd.PartialGenotypes._fields)
    assert "#define MTR_ABI_VERSION 5" in hdr or re.search(r"MTR_ABI_VERSION\s+5", hdr)
    src = open(os.path.join(ROOT, "mtr_amd", "csrc", "motif_ext.h")).read()
    assert "hip/" not in src and "__global__" not in src and "threadIdx" not in src      # nothing of HIP in the lane's definition
