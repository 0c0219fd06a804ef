"""The host side of the allele consensus on the CPU: format_allele_consensus, join_sparse_genotypes, join_windows and Genotypes.to_sparse on numpy
arrays and CPU tensors (no library call)."""
import numpy as np
import pytest

import mtr_amd

LOCI = [("ACGT", "CAG", "TTGA"), ("GGCA", b"GAA", "CATG")]


def _cons(conv=np.asarray):
    # locus 0: both alleles (CAGCAA, and an empty sequence); locus 1: allele 0 only
    return mtr_amd.AlleleConsensus(conv(np.array([0, 6, 6, 9, 9], np.int64)), conv(np.array([1, 0, 2, 1, 0, 0, 2, 0, 0], np.uint8)), conv(np.arange(9, dtype=np.int32)),
                                   conv(np.array([4, 7, 2, -1], np.int32)), conv(np.array([6, 0, 3, 0], np.int32)), conv(np.array([5, 3, 2, 0], np.int32)),
                                   conv(np.array([4, 1, 1, 0], np.int32)), conv(np.array([0, 1, 0, 0], np.int32)))


def test_one_line_per_called_allele():
    want = b"0\t0\t5\t4\t0\t6\tCAGCAA\tCAG\n0\t1\t3\t1\t1\t0\t.\tCAG\n1\t0\t2\t1\t0\t3\tGAA\tGAA\n"
    assert mtr_amd.format_allele_consensus(LOCI, _cons()) == want
    torch = pytest.importorskip("torch")
    assert mtr_amd.format_allele_consensus(LOCI, _cons(lambda a: torch.from_numpy(a))) == want
    with pytest.raises(mtr_amd.MtrError, match="4 alleles for 1 loci"):
        mtr_amd.format_allele_consensus(LOCI[:1], _cons())


def _dense(n, m, seed):
    rng = np.random.default_rng(seed)
    sp = (rng.random((n, m)) < 0.4).astype(np.uint8)
    full = lambda dt, *tail: (rng.integers(1, 50, size=(n, m) + tail) * sp.reshape((n, m) + (1,) * len(tail))).astype(dt)      # noqa: E731
    return mtr_amd.Genotypes(sp, full(np.uint8) % 2, full(np.int32, 2), full(np.int32, 2), full(np.int32, 8), full(np.int32), full(np.float32))


@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy", "torch"])
def test_to_sparse_is_the_spanning_rows_in_order_and_to_dense_undoes_it(as_tensor):
    gt = _dense(7, 5, 3)
    if as_tensor:
        torch = pytest.importorskip("torch")
        src = mtr_amd.Genotypes(*[torch.from_numpy(c) for c in gt])
    else:
        src = gt
    sg = src.to_sparse()
    host = lambda t: t.numpy() if hasattr(t, "detach") else t      # noqa: E731
    at = np.flatnonzero(gt.spanning.reshape(-1))
    assert (sg.n_reads, sg.n_loci, sg.candidates) == (7, 5, len(at)) and len(at) > 5
    assert host(sg.read).dtype == np.int32 and host(sg.read).tolist() == (at // 5).tolist() and host(sg.locus).tolist() == (at % 5).tolist()
    for k, c in enumerate(gt):
        got = host(sg[4 + k])
        assert got.dtype == c.dtype and np.array_equal(got, c.reshape((35,) + c.shape[2:])[at]), mtr_amd.Genotypes._fields[k]
    if as_tensor:
        back = sg.to_dense()
        assert all(np.array_equal(b.numpy(), c) for b, c in zip(back, gt))


def test_the_joins_do_what_the_docstring_said_to_do_by_hand():
    torch = pytest.importorskip("torch")
    parts = [mtr_amd.Genotypes(*[torch.from_numpy(c) for c in _dense(n, 4, seed)]).to_sparse() for n, seed in ((3, 1), (5, 2), (2, 4))]
    wins = []
    for k, p in enumerate(parts):
        lens = (p.window[:, 1] - p.window[:, 0]).abs().long() % 7
        off = torch.zeros(len(lens) + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(lens, 0)
        wins.append(mtr_amd.GenotypeWindows(off, torch.full((int(off[-1]),), k, dtype=torch.uint8)))
    sg, win = mtr_amd.join_sparse_genotypes(parts), mtr_amd.join_windows(wins)
    assert (sg.n_reads, sg.n_loci) == (10, 4) and sg.candidates == sum(p.candidates for p in parts)
    assert torch.equal(sg.read, torch.cat([parts[0].read, parts[1].read + 3, parts[2].read + 8])) and sg.read.dtype == torch.int32
    for k in range(3, 11):
        assert torch.equal(sg[k], torch.cat([p[k] for p in parts])), mtr_amd.SparseGenotypes._fields[k]
    key = sg.read.long() * 4 + sg.locus.long()
    assert (key[1:] > key[:-1]).all()                                               # the joined rows stay sorted
    assert win.off.numel() == sg.read.numel() + 1 and int(win.off[-1]) == win.bases.numel() == sum(int(w.off[-1]) for w in wins)
    assert torch.equal(win.off[1:] - win.off[:-1], torch.cat([w.off[1:] - w.off[:-1] for w in wins]))
    assert torch.equal(win.bases, torch.cat([w.bases for w in wins]))
    np_join = mtr_amd.join_windows([mtr_amd.GenotypeWindows(w.off.numpy(), w.bases.numpy()) for w in wins])
    assert np.array_equal(np_join.off, win.off.numpy()) and np.array_equal(np_join.bases, win.bases.numpy())
    with pytest.raises(mtr_amd.MtrError, match="n_loci differ"):
        mtr_amd.join_sparse_genotypes([parts[0], parts[1]._replace(n_loci=5)])
    with pytest.raises(mtr_amd.MtrError, match="nothing to join"):
        mtr_amd.join_windows([])
