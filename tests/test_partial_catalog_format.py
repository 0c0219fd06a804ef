"""format_sparse_partial_genotypes, SparsePartialGenotypes.to_dense and partial_support on a SparsePartialGenotypes (mtr_amd/__init__.py) on
hand-made CPU tensors and numpy columns, against the dense forms of tests/test_partial_format.py; and the declarations of the partial genotype at
catalogue scale: the header, EXPORTS, the ctypes mirror of mtr_partial_catalog_dst."""
import os
import re

import pytest

import mtr_amd
from tests.test_partial_format import LOCI, _calls, _pg

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spg(pg=None, candidates=5):
    """the partial rows of a dense result as the catalogue call returns them"""
    pg = pg or _pg()
    n, m = pg.partial.shape
    at = torch.nonzero(pg.partial)
    cols = [c[at[:, 0], at[:, 1]] for c in pg]
    return mtr_amd.SparsePartialGenotypes(n, m, at[:, 0].to(torch.int32), at[:, 1].to(torch.int32), *cols, candidates)


def test_the_sparse_lines_are_the_dense_lines():
    ids, lens = ["r0", b"r1", "r2"], [60, 70, 50]
    want = mtr_amd.format_partial_genotypes(ids, lens, LOCI, _pg())
    assert want.count(b"\n") == 4
    assert mtr_amd.format_sparse_partial_genotypes(ids, lens, LOCI, _spg()) == want
    as_numpy = mtr_amd.SparsePartialGenotypes(3, 2, *[c.numpy() for c in _spg()[2:11]], 5)
    assert mtr_amd.format_sparse_partial_genotypes(ids, lens, LOCI, as_numpy) == want
    empty = mtr_amd.SparsePartialGenotypes(3, 2, *[c[:0] for c in _spg()[2:11]], 0)
    assert mtr_amd.format_sparse_partial_genotypes(ids, lens, LOCI, empty) == b""
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.format_sparse_partial_genotypes(ids, lens[:2], LOCI, _spg())
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.format_sparse_partial_genotypes(ids, lens, LOCI[:1], _spg())


def test_to_dense_gives_the_dense_columns_back():
    back = _spg().to_dense()
    assert isinstance(back, mtr_amd.PartialGenotypes)
    # the dense call writes zeros where a row is not partial; _pg()'s rows do
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(back, _pg()))
    empty = mtr_amd.SparsePartialGenotypes(3, 2, *[c[:0] for c in _spg()[2:11]], 0).to_dense()
    assert all(c.shape[:2] == (3, 2) and not bool(c.any()) for c in empty)


@pytest.mark.parametrize("larger", [None, (8, 7), (7, 0), (13, -1), (0, 0)])
@pytest.mark.parametrize("min_ratio", [0.0, 0.96])
def test_partial_support_of_the_sparse_rows_is_that_of_the_dense_ones(larger, min_ratio):
    calls = _calls(larger) if larger else None
    s, d = mtr_amd.partial_support(_spg(), calls, min_ratio), mtr_amd.partial_support(_pg(), calls, min_ratio)
    for a, b in zip(s, d):
        assert (a is None and b is None) or (torch.equal(a, b) and a.dtype == b.dtype), (s, d)
    assert (s.n_beyond is None) == (larger is None)


def test_partial_support_of_sparse_rows_at_its_edges():
    assert mtr_amd.partial_support(_spg(), _calls((8, 7))).n_beyond.tolist() == [1, 0] and mtr_amd.partial_support(_spg()).max_copies.tolist() == [13, 0]
    empty = mtr_amd.SparsePartialGenotypes(3, 2, *[c[:0] for c in _spg()[2:11]], 0)
    s = mtr_amd.partial_support(empty, _calls((1, 1)))
    assert (s.n_partial.tolist(), s.n_open.tolist(), s.max_copies.tolist(), s.n_beyond.tolist()) == ([0, 0], [0, 0], [0, 0], [0, 0])
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.partial_support(_spg(), mtr_amd.AlleleCalls(*[c[:1] if c.dim() == 2 else c for c in _calls((1, 1))]))
    # two batches joined as the docstring says: the second batch's reads follow the first's
    a, b = _spg(), _spg()
    joined = mtr_amd.SparsePartialGenotypes(6, 2, torch.cat([a.read, b.read + 3]), *[torch.cat([x, y]) for x, y in zip(a[3:11], b[3:11])], 10)
    s = mtr_amd.partial_support(joined, _calls((8, 7)))
    assert (s.n_partial.tolist(), s.n_open.tolist(), s.max_copies.tolist(), s.n_beyond.tolist()) == ([4, 4], [4, 2], [13, 0], [2, 0])
    assert bool((joined.read[1:] >= joined.read[:-1]).all())


def test_the_declarations_agree():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    for name in ("mtr_genotype_partial_catalog_device", "mtr_genotype_partial_catalog_copy_device"):
        assert re.search(r"mtr_status " + name + r"\(mtr_ctx \*ctx", hdr) and name in mtr_amd.EXPORTS, name
    body = re.search(r"typedef struct mtr_partial_catalog_dst \{(.*?)\} mtr_partial_catalog_dst;", hdr, re.S).group(1)
    assert re.findall(r"\*?(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in mtr_amd.CPartialCatalogDst._fields_]
    assert mtr_amd.CPartialCatalogDst._fields_[2][1] is mtr_amd.CPartialDst
    assert list(mtr_amd.SparsePartialGenotypes._fields) == ["n_reads", "n_loci", "read", "locus"] + list(mtr_amd.PartialGenotypes._fields) + ["candidates"]
    assert re.search(r"MTR_ABI_VERSION\s+5", hdr)
    assert "add" in mtr_amd.SparsePartialGenotypes.__doc__ and "torch.cat" in mtr_amd.SparsePartialGenotypes.__doc__      # the join rule
