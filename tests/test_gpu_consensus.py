"""The allele consensus on the MI355X (mtr_extract_windows_device, mtr_allele_consensus_device, Engine.genotype_windows / allele_consensus, the
kernels of mtr_amd/csrc/consensus.hip.inc).

Truth is tests/consensus_ref.py, the definition of include/mtr_hip.h in plain Python; tests/test_consensus_ref.py holds it to hand-worked answers
and shows that the inputs of tests/consensus_cases.py are not degenerate and that its consensus is the true allele on the seeds used here.
Everything is exact equality: every column, every dtype, every shape."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import mtr_amd
from tests import consensus_cases as cc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", eng.device))


def _inputs(eng, case):
    sg = SimpleNamespace(n_loci=case["n_loci"], read=_dev(eng, case["read"]), locus=_dev(eng, case["locus"]))
    win = mtr_amd.GenotypeWindows(_dev(eng, case["win_off"]), _dev(eng, case["win_bases"]))
    calls = SimpleNamespace(support_off=_dev(eng, case["support_off"]), read=_dev(eng, case["sup_read"]), allele=_dev(eng, case["allele"]), zygosity=_dev(eng, case["zygosity"]))
    return sg, win, calls


def _assert_cons(got, want, what=""):
    for name, g, w in zip(mtr_amd.AlleleConsensus._fields, (t.cpu().numpy() for t in got), want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError((what, name, at.tolist(), g[tuple(at)].tolist(), w[tuple(at)].tolist()))


@pytest.mark.parametrize("name", sorted(cc.all_cases()))
def test_every_column_equals_the_reference(eng, name):
    case, want = cc.expected()[name]
    got = eng.allele_consensus(*_inputs(eng, case), band_extra=case["band_extra"])
    _assert_cons(got, want, name)
    again = eng.allele_consensus(*_inputs(eng, case), band_extra=case["band_extra"])
    assert all(torch.equal(x, y) for x, y in zip(got, again)), name


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------
def _window_rows():
    rng = np.random.default_rng(21)
    reads = [cc.seq(rng, n) for n in (1, 15, 16, 17, 33, 64, 200, 5)]
    rows = []
    for lo in range(0, 18):                             # a window starting at every residue of a packed word, in both orientations
        rows += [(6, lo, lo + 37, 0), (6, lo, lo + 37, 1)]
    rows += [(0, 0, 1, 1), (0, 1, 1, 0), (1, 0, 15, 1), (2, 0, 16, 1), (3, 1, 17, 0), (4, 0, 33, 1), (5, 0, 64, 0), (5, 15, 49, 1), (7, 2, 2, 1), (6, 0, 200, 1)]
    rows.sort()
    return reads, rows


def _rows_namespace(eng, rows):
    col = lambda k, dt: _dev(eng, np.array([r[k] for r in rows], dt).reshape(len(rows)))      # noqa: E731
    return SimpleNamespace(read=col(0, np.int32), orientation=col(3, np.uint8), window=_dev(eng, np.array([[r[1], r[2]] for r in rows], np.int32).reshape(len(rows), 2)))


def test_the_windows_equal_slicing_on_the_host(eng):
    reads, rows = _window_rows()
    eng.upload(reads)
    win = eng.genotype_windows(_rows_namespace(eng, rows))
    want = [cc.oriented_window(reads[r], lo, hi, o) for r, lo, hi, o in rows]
    assert win.off.dtype == torch.int64 and win.bases.dtype == torch.uint8
    assert win.off.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()
    assert win.bases.cpu().numpy().tolist() == np.concatenate(want).tolist()
    none = eng.genotype_windows(_rows_namespace(eng, []))
    assert none.off.cpu().tolist() == [0] and none.bases.numel() == 0


def test_the_windows_protocol_and_the_destination_stays(eng):
    reads, rows = _window_rows()
    fresh = mtr_amd.Engine()
    with pytest.raises(mtr_amd.MtrError, match="no batch uploaded"):
        fresh.genotype_windows(_rows_namespace(fresh, rows))
    fresh.close()
    eng.upload(reads)
    for bad, word in (((8, 0, 1, 0), "row 2"), ((-1, 0, 1, 0), "row 2"), ((6, 5, 201, 0), "row 2"), ((6, 9, 8, 1), "row 2"), ((6, -1, 8, 1), "row 2")):
        with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: {word}:"):
            eng.genotype_windows(_rows_namespace(eng, rows[:2] + [bad] + rows[2:]))
    ns = _rows_namespace(eng, rows)
    R, T = len(rows), sum(r[2] - r[1] for r in rows)
    dev = torch.device("cuda", eng.device)
    off, bases = torch.full((R + 1,), 77, dtype=torch.int64, device=dev), torch.full((T,), 77, dtype=torch.uint8, device=dev)
    nb = C.c_int64()
    call = lambda dst: eng.lib.mtr_extract_windows_device(eng.h, ns.read.data_ptr(), ns.orientation.data_ptr(), ns.window.data_ptr(), R, None, dst, C.byref(nb))      # noqa: E731
    torch.cuda.synchronize()
    assert call(None) == 0 and nb.value == T
    for cap_rows, cap_bases in ((R - 1, T), (R, T - 1)):
        assert mtr_amd.STATUS[call(C.byref(mtr_amd.CWindowsDst(off.data_ptr(), bases.data_ptr(), cap_rows, cap_bases)))] == "MTR_ERR_OVERFLOW" and nb.value == T
    assert mtr_amd.STATUS[call(C.byref(mtr_amd.CWindowsDst(None, bases.data_ptr(), R, T)))] == "MTR_ERR_BAD_ARG"
    assert mtr_amd.STATUS[eng.lib.mtr_extract_windows_device(eng.h, ns.read.data_ptr(), None, ns.window.data_ptr(), R, None, None, C.byref(nb))] == "MTR_ERR_BAD_ARG"
    assert (off == 77).all() and (bases == 77).all()
    assert call(C.byref(mtr_amd.CWindowsDst(off.data_ptr(), bases.data_ptr(), R, T))) == 0
    good = eng.genotype_windows(ns)
    assert torch.equal(off, good.off) and torch.equal(bases, good.bases)


# ---- from reads to sequences --------------------------------------------------------------------------------------------------------------------
def _pipeline(eng, batches, loci):
    parts, wins = [], []
    for reads in batches:
        eng.upload(reads)
        sg = eng.genotype_catalog(loci, 1)
        parts.append(sg)
        wins.append(eng.genotype_windows(sg))
    sg, win = mtr_amd.join_sparse_genotypes(parts), mtr_amd.join_windows(wins)
    calls = eng.call_alleles(sg, "bases")
    return sg, win, calls, eng.allele_consensus(sg, win, calls, band_extra=cc.TRUTH_EXTRA)


@pytest.mark.parametrize("seed", cc.TRUTH_SEEDS)
def test_from_reads_to_the_true_alleles_in_one_batch_and_in_two(eng, seed):
    reads, loci, truth = cc.truth_reads(seed), cc.truth_loci(), cc.truth_alleles()
    sg, win, calls, cons = _pipeline(eng, [reads], loci)
    n = 2 * cc.TRUTH_READS
    assert sg.read.cpu().tolist() == list(range(n)) and sg.locus.cpu().tolist() == [0] * n and sg.orientation.cpu().tolist() == [k % 2 for k in range(n)]
    flat = [w for ws in cc.truth_windows(seed) for w in ws]
    assert win.off.cpu().tolist() == [0] + np.cumsum([len(w) for w in flat]).tolist() and win.bases.cpu().numpy().tolist() == np.concatenate(flat).tolist()
    assert calls.zygosity.cpu().tolist() == [2, 0] and calls.call_support.cpu().tolist()[0] == [cc.TRUTH_READS] * 2
    off = cons.off.cpu().tolist()
    assert off[2:] == [off[2]] * 3 and cons.backbone_read.cpu().tolist()[2:] == [-1, -1]
    for a in (0, 1):
        assert cons.bases[off[a]:off[a + 1]].cpu().tolist() == truth[a].tolist(), (seed, a)
    _, want = cc.expected()[f"truth{seed}"]              # the same windows in the same member order: the reference's columns (its reads are numbered otherwise)
    for k in (0, 1, 2, 4, 5, 6, 7):
        assert np.array_equal(cons[k].cpu().numpy()[:len(want[k])], want[k]), mtr_amd.AlleleConsensus._fields[k]
    text = mtr_amd.format_allele_consensus(loci, cons).decode().splitlines()
    assert len(text) == 2 and text[0].split("\t")[6] == "".join(cc.LETTERS[c] for c in truth[0]) and text[1].split("\t")[:2] == ["0", "1"]
    dense = eng.genotype_loci(loci, 1).to_sparse()        # (the batch is still resident) the dense result enters the same path
    assert all(torch.equal(x, y) for x, y in zip(dense[2:11], sg[2:11])) and (dense.n_reads, dense.n_loci) == (sg.n_reads, sg.n_loci)
    two = _pipeline(eng, [reads[:7], reads[7:]], loci)
    assert two[0].n_reads == n and all(torch.equal(x, y) for x, y in zip(two[0][2:11], sg[2:11]))
    assert all(torch.equal(x, y) for x, y in zip(two[1], win)) and all(torch.equal(x, y) for x, y in zip(two[3], cons))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_the_refusals_write_nothing_and_the_next_call_succeeds(eng):
    case, want = cc.expected()["members"]
    sg, win, calls = _inputs(eng, case)
    swapped = case["read"].copy()
    swapped[[4, 5]] = swapped[[5, 4]]
    locus_swapped = case["locus"].copy()
    locus_swapped[[4, 5]] = locus_swapped[[5, 4]]
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: row 5 is out of order"):
        eng.allele_consensus(SimpleNamespace(n_loci=sg.n_loci, read=_dev(eng, swapped), locus=_dev(eng, locus_swapped)), win, calls, band_extra=8)
    lost = case["sup_read"].copy()
    lost[7] = int(case["read"].max()) + 1
    with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: support entry 7 \(read \d+\) has no row"):
        eng.allele_consensus(sg, win, SimpleNamespace(support_off=calls.support_off, read=_dev(eng, lost), allele=calls.allele, zygosity=calls.zygosity), band_extra=8)
    for extra in (-1, mtr_amd.CONS_MAX_EXTRA + 1):
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: band_extra"):
            eng.allele_consensus(sg, win, calls, band_extra=extra)
    G, T = 2 * case["n_loci"], len(want[1])
    dev = torch.device("cuda", eng.device)
    shapes = ((G + 1, torch.int64), (T, torch.uint8), (T, torch.int32)) + ((G, torch.int32),) * 5
    cols = [torch.full((n,), 77, dtype=t, device=dev) for n, t in shapes]
    src = mtr_amd.CConsensusSrc(sg.read.data_ptr(), sg.locus.data_ptr(), win.off.data_ptr(), win.bases.data_ptr(), calls.support_off.data_ptr(), calls.read.data_ptr(),
                                calls.allele.data_ptr(), calls.zygosity.data_ptr(), sg.read.numel(), win.bases.numel(), calls.read.numel(), case["n_loci"])
    nb = C.c_int64()
    call = lambda dst, extra=8: eng.lib.mtr_allele_consensus_device(eng.h, C.byref(src), extra, None, dst, C.byref(nb))      # noqa: E731
    ptrs = [c.data_ptr() for c in cols]
    torch.cuda.synchronize()
    assert call(None) == 0 and nb.value == T
    for cap_alleles, cap_bases in ((G - 1, T), (G, T - 1)):
        assert mtr_amd.STATUS[call(C.byref(mtr_amd.CConsensusDst(*ptrs, cap_alleles, cap_bases)))] == "MTR_ERR_OVERFLOW" and nb.value == T
    assert mtr_amd.STATUS[call(C.byref(mtr_amd.CConsensusDst(*ptrs[:2], None, *ptrs[3:], G, T)))] == "MTR_ERR_BAD_ARG"
    assert mtr_amd.STATUS[call(C.byref(mtr_amd.CConsensusDst(*ptrs, G, T)), 65)] == "MTR_ERR_BAD_ARG"
    assert all((c == 77).all() for c in cols)
    assert call(C.byref(mtr_amd.CConsensusDst(*ptrs, G, T))) == 0
    _assert_cons(cols, want, "after the refusals")
