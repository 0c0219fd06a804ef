"""The catalogue genotype's Python layer on the CPU: format_sparse_genotypes against format_genotypes of the dense form (SparseGenotypes.to_dense),
the seed length picked by default and the argument errors raised before the library is called, and the declarations - the header, EXPORTS, the
ctypes mirror of mtr_catalog_dst."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd
from tests import catalog_cases as cc
from tests import catalog_ref as cref
from tests import flank_ref as fref

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sparse(rows, n, m, candidates):
    col = lambda k, dtype: torch.tensor(np.array([r[k] for r in rows], dtype).reshape((len(rows),) + np.shape(rows[0][k]) if rows else (0,)))      # noqa: E731
    return mtr_amd.SparseGenotypes(n, m, col(0, np.int32), col(1, np.int32), torch.ones(len(rows), dtype=torch.uint8), col(2, np.uint8), col(3, np.int32),
                                   col(4, np.int32), col(5, np.int32), col(6, np.int32), col(7, np.float32), candidates)


def test_the_sparse_text_is_the_dense_text():
    loci, reads = cc.cases(1, 8)
    loci = loci[:8]
    rows, cands = cref.genotype(reads, loci, 1, 8)
    sg = _sparse(rows, len(reads), len(loci), len(cands))
    dense = sg.to_dense()
    assert dense.spanning.shape == (len(reads), len(loci)) and int(dense.spanning.sum()) == len(rows) and dense.fields.shape == (len(reads), len(loci), 8)
    want, _ = fref.genotype(reads, loci, 1)
    assert all(np.array_equal(d.numpy(), w) for d, w in zip(dense, want))
    ids, lens, texts = [f"read{i}" for i in range(len(reads))], [len(r) for r in reads], [tuple(fref.text(s) for s in locus) for locus in loci]
    text = mtr_amd.format_sparse_genotypes(ids, lens, texts, sg)
    assert text == mtr_amd.format_genotypes(ids, lens, texts, dense) and text.count(b"\n") == len(rows) >= 30
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.format_sparse_genotypes(ids[:-1], lens, texts, sg)
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.format_sparse_genotypes(ids, lens, texts[:-1], sg)


def test_the_default_seed_length_and_its_errors():
    f = lambda n: "ACGT" * (n // 4) + "ACGT"[:n % 4]      # noqa: E731
    assert mtr_amd.pick_seed_len([(f(48), "CAG", f(50))], 3) == 12 and mtr_amd.pick_seed_len([(f(64), "CAG", f(64))], 3) == 16
    assert mtr_amd.pick_seed_len([(f(64), "CAG", f(64)), (f(20), "A", f(17))], 0) == 16 and mtr_amd.pick_seed_len([(f(64), "CAG", f(17))], 1) == 8
    with pytest.raises(mtr_amd.MtrError, match="locus 1, right flank"):
        mtr_amd.pick_seed_len([(f(64), "CAG", f(64)), (f(64), "CAG", f(31))], 3)
    with pytest.raises(mtr_amd.MtrError, match="max_flank_dist"):
        mtr_amd.pick_seed_len([(f(64), "CAG", f(64))], -1)
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.pick_seed_len([], 1)


def test_the_declarations():
    hdr = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    for name in ("mtr_genotype_catalog_device", "mtr_genotype_catalog_copy_device", "mtr_call_alleles_rows_device"):
        assert re.search(rf"mtr_status {name}\(mtr_ctx \*ctx", hdr) and name in mtr_amd.EXPORTS
    assert "#define MTR_ABI_VERSION 5" in hdr and "mtr_test_catalog_stats" in mtr_amd.EXPORTS
    assert "mtr_status mtr_test_catalog_stats(mtr_ctx *ctx" in open(os.path.join(ROOT, "include", "mtr_hip_test.h")).read()
    assert C.sizeof(mtr_amd.CCatalogDst) == 2 * 8 + C.sizeof(mtr_amd.CGenotypesDst) == 80
    assert mtr_amd.SparseGenotypes._fields == ("n_reads", "n_loci", "read", "locus") + mtr_amd.Genotypes._fields + ("candidates",)


def test_the_checks_of_sparse_rows_before_the_library_is_called():
    sg = mtr_amd.SparseGenotypes(2, 1, *[torch.zeros(s, dtype=t) for s, t in (((1,), torch.int32), ((1,), torch.int32), ((1,), torch.uint8), ((1,), torch.uint8), ((1, 2), torch.int32),
                                                                              ((1, 2), torch.int32), ((1, 8), torch.int32), ((1,), torch.int32), ((1,), torch.float32))], 0)
    with pytest.raises(mtr_amd.MtrError, match="GPU tensors"):
        mtr_amd.sparse_rows_args(sg, 0)
    with pytest.raises(mtr_amd.MtrError, match="locus"):
        mtr_amd.sparse_rows_args(sg._replace(locus=sg.locus.long()), 0)
    with pytest.raises(mtr_amd.MtrError, match="window"):
        mtr_amd.sparse_rows_args(sg._replace(window=torch.zeros((2, 2), dtype=torch.int32)), 0)
    with pytest.raises(mtr_amd.MtrError, match="n_loci"):
        mtr_amd.sparse_rows_args(sg._replace(n_loci=0), 0)
