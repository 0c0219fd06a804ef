"""The partial genotype on the MI355X (mtr_genotype_partial_device, Engine.genotype_partial, the kernels of mtr_amd/csrc/partial.hip.inc over
those of flank_search.hip.inc).

Truth is tests/partial_ref.py on the seeded inputs of tests/partial_cases.py (tests/test_partial_ref.py shows, on the CPU, that they are not
degenerate): motifs of 1, 2, 3, 4, 5, 8, 9, 16, 17 and 32 bases, all four slots, windows starting and ending at every residue of a word, K = 0
and K = 3, and the scores (1, 1, 1), (2, 3, 2) and (5, 4, 7).  Every column must equal the reference.  The last score set lies outside what the
search's checks admit (mismatch and indel are at most 3) and the call's checks are the search's: for it the call must answer MTR_ERR_BAD_ARG
and write nothing; the lane's function itself is held to (5, 4, 7) by tests/motif_ext_check.cpp."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import flank_ref as fref
from tests import motif_search_ref as ref
from tests import partial_cases as pc
from tests import partial_ref as pref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _assert_columns(pg, want, what=""):
    for name, g, w in zip(mtr_amd.PartialGenotypes._fields, (t.cpu().numpy() for t in pg), want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            r, k = int(at[0]), int(at[1])
            raise AssertionError((what, name, r, k, g[r, k].tolist(), w[r, k].tolist(), [c[r, k].tolist() for c in want]))


@pytest.mark.parametrize("scores", pc.SCORES, ids=str)
@pytest.mark.parametrize("K", pc.KS)
def test_every_column_on_the_grid(eng, K, scores):
    eng.upload(pc.BATCH)
    if max(scores[1:]) > 3:                                      # the search's checks: mismatch and indel in 1..3
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
            eng.genotype_partial(pc.TEXTS, K, *scores, max_tail=pc.MAX_TAIL)
        return
    want = pc.want(K, scores)
    pg = eng.genotype_partial(pc.TEXTS, K, *scores, max_tail=pc.MAX_TAIL)
    _assert_columns(pg, want, f"K = {K}, {scores}")
    again = eng.genotype_partial(pc.TEXTS, K, *scores, max_tail=pc.MAX_TAIL)
    assert all(torch.equal(a, b) for a, b in zip(pg, again))
    ids, lens = [f"r{i}" for i in range(len(pc.BATCH))], [len(r) for r in pc.BATCH]
    text = mtr_amd.format_partial_genotypes(ids, lens, pc.TEXTS, pg)
    assert text == mtr_amd.format_partial_genotypes(ids, lens, pc.TEXTS, mtr_amd.PartialGenotypes(*want)) and text.count(b"\n") == int(want[0].sum())
    assert text.count(b">=") == int(want[6].sum())


@pytest.mark.parametrize("n_loci", [1, 2, 7])
def test_fewer_loci_in_one_call(eng, n_loci):
    """a row depends on its own read and locus alone: the columns are the full reference's first n_loci loci"""
    eng.upload(pc.BATCH)
    _assert_columns(eng.genotype_partial(pc.TEXTS[:n_loci], 3, max_tail=pc.MAX_TAIL), [c[:, :n_loci] for c in pc.want(3)], f"{n_loci} loci")


def test_max_tail_moves_open_and_nothing_else(eng):
    eng.upload(pc.BATCH)
    want = pc.want(3)
    for max_tail in (0, 25):
        pg = eng.genotype_partial(pc.TEXTS, 3, max_tail=max_tail)
        _assert_columns(pg[:6], want[:6], f"max_tail = {max_tail}")
        assert np.array_equal(pg.open.cpu().numpy(), ((want[0] == 1) & (want[4][:, :, 5] <= max_tail)).astype(np.uint8))


@pytest.mark.parametrize("tasks", [0, 1, 63, 64, 65, 129])
def test_batches_by_their_number_of_tasks(eng, tasks):
    """all tasks are of one variant: 0, 1, 2 and 3 wavefronts, full and not.  Without a task no extension is launched and the rows are zeros"""
    reads = pc.task_batch(tasks)
    want = pref.genotype_partial(reads, pc.LOCI[2:3], 0, max_tail=pc.MAX_TAIL)
    assert int((want[3][:, :, 1] > want[3][:, :, 0]).sum()) == tasks == int(want[0].sum())
    eng.upload(reads)
    pg = eng.genotype_partial(pc.TEXTS[2:3], 0, max_tail=pc.MAX_TAIL)
    _assert_columns(pg, want, f"{tasks} tasks")
    if tasks == 0:
        assert all(not bool(c.any()) for c in pg)


def test_consistent_with_the_genotype_on_the_same_batch(eng):
    eng.upload(pc.BATCH)
    for K in pc.KS:
        pg, gt = eng.genotype_partial(pc.TEXTS, K), eng.genotype_loci(pc.TEXTS, K)
        assert not bool((pg.partial & gt.spanning).any())
        pats = [fref.text(q) for A, _, B in pc.LOCI for q in (A, B, ref.revcomp(A), ref.revcomp(B))]      # the four slots of every locus
        fl = eng.search_flanks(pats, both_strands=False)
        near = (fl.dist.reshape(len(pc.BATCH), len(pc.TEXTS), 4) <= K).any(dim=2)
        assert torch.equal(pg.partial != 0, (gt.spanning == 0) & near), K
        assert int(gt.spanning.sum()) >= 2 and int(pg.partial.sum()) >= 300


# ---- protocol ---------------------------------------------------------------------------------------------------------------------------
def _raw(eng, loci, K=2, scores=(1, 1, 1), max_tail=10, off=None):
    flat = [s for locus in loci for s in locus]
    data, o = mtr_amd.pack_ids(flat)
    if off is not None:
        o = np.array(off, np.int64)
    nr = C.c_int64(-7)
    st = eng.lib.mtr_genotype_partial_device(eng.h, data.ctypes.data, o.ctypes.data, len(loci), K, *scores, max_tail, None, C.byref(nr))
    return mtr_amd.STATUS.get(st, st), int(nr.value), eng.lib.mtr_last_error(eng.h).decode()


def test_the_argument_errors_and_the_batch_stays_usable(eng):
    reads = pc.task_batch(65)
    eng.upload(reads)
    ok = pc.TEXTS[2]
    long_read_short_motif = ("ACGTACGTAC", "ACGT" * 8, "TTGACCGATA")
    for kw, word in ((dict(loci=[]), "n_loci"), (dict(loci=[ok], off=[0, 10, 9, 20]), "decreases"), (dict(loci=[ok], scores=(0, 1, 1)), "gain"),
                     (dict(loci=[ok], scores=(5, 4, 7)), "mismatch"), (dict(loci=[ok], scores=(1, 1, 0)), "indel"), (dict(loci=[ok, ("ACGT", "", "ACGT")]), "motif 1"),
                     (dict(loci=[("ACGT", "CAN", "ACGT")]), "ACGT"), (dict(loci=[ok, ("", "CAG", "ACGT")]), "locus 1, left flank"), (dict(loci=[ok], K=-1), "max_flank_dist"),
                     (dict(loci=[ok, long_read_short_motif, ("ACGT", "A" * 33, "ACGT")]), "locus 2"), (dict(loci=[ok], max_tail=-1), "max_tail"),
                     (dict(loci=[("ACGT", "A" * 33, "ACGT")], max_tail=-1), "locus 0"), (dict(loci=[("ACGT", "A" * 33, "ACGT")], K=-1), "max_flank_dist"),
                     (dict(loci=[("ACGT", "A" * 500, "ACGT")]), "motif 0")):
        st, R, msg = _raw(eng, **kw)
        assert st == "MTR_ERR_BAD_ARG" and word in msg and R == 0, (kw, st, msg)
    assert _raw(eng, [ok, long_read_short_motif])[:2] == ("MTR_OK", 2 * len(reads))                    # the size call; 32 bases are taken
    with pytest.raises(mtr_amd.MtrError):
        eng.genotype_partial([("ACGT", "CAG")], 1)
    # a destination too small, and a NULL column: nothing written
    dev = torch.device("cuda", eng.device)
    R = len(reads)
    shapes = ((R, torch.uint8), (R, torch.uint8), (R, torch.int32), (2 * R, torch.int32), (6 * R, torch.int32), (R, torch.float32), (R, torch.uint8))
    cols = [torch.full((n,), 77, dtype=t, device=dev) for n, t in shapes]
    torch.cuda.synchronize()
    data, o = mtr_amd.pack_ids(list(ok))
    nr = C.c_int64()
    call = lambda dst: mtr_amd.STATUS[eng.lib.mtr_genotype_partial_device(eng.h, data.ctypes.data, o.ctypes.data, 1, 0, 1, 1, 1, 10, C.byref(dst), C.byref(nr))]      # noqa: E731
    ptrs = [c.data_ptr() for c in cols]
    assert call(mtr_amd.CPartialDst(*ptrs, R - 1)) == "MTR_ERR_OVERFLOW"
    for k in range(7):
        assert call(mtr_amd.CPartialDst(*ptrs[:k], None, *ptrs[k + 1:], R)) == "MTR_ERR_BAD_ARG", k
    torch.cuda.synchronize()
    assert all(bool((c == 77).all()) for c in cols)
    assert call(mtr_amd.CPartialDst(*ptrs, R)) == "MTR_OK" and int(nr.value) == R
    want = pref.genotype_partial(reads, pc.LOCI[2:3], 0, max_tail=10)
    assert all(np.array_equal(c.cpu().numpy().reshape(w.shape), w) for c, w in zip(cols, want))
    _assert_columns(eng.genotype_partial([ok], 0), want, "after the errors")


def test_no_batch():
    e = mtr_amd.Engine()
    try:
        st, _, msg = _raw(e, [("ACGT", "CAG", "ACGT")])
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
        st, _, msg = _raw(e, [], K=-1)                                                                 # the batch is asked for first
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
    finally:
        e.close()


def test_no_dp_too_large_and_no_dependence_on_the_lane_rows_knob(monkeypatch):
    """under a WrapDPsize at which the genotype refuses the batch the partial genotype answers: it stores no cell; and windows of up to 288
    bases extend with the search's lane path cut at 64 rows"""
    sub = pc.BATCH[::7] + pc.EXTRA
    want = pref.genotype_partial(sub, pc.LOCI[7:], 3, max_tail=pc.MAX_TAIL)
    assert int((want[3][:, :, 1] - want[3][:, :, 0]).max()) > 4 * 64
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(33 * 300))
    monkeypatch.setenv("MTR_TEST_MOTIF_LANE_ROWS", "64")
    e = mtr_amd.Engine()
    try:
        e.upload(sub)
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
            e.genotype_loci(pc.TEXTS[7:], 3)
        _assert_columns(e.genotype_partial(pc.TEXTS[7:], 3, max_tail=pc.MAX_TAIL), want, "lane rows 64")
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        monkeypatch.delenv("MTR_TEST_MOTIF_LANE_ROWS")
        mtr_amd.Engine().close()                                                                     # the device's limit back to the built-in one


# ---- nothing else moves -------------------------------------------------------------------------------------------------------------------
def test_a_partial_genotype_leaves_the_run_and_its_report_alone(eng):
    reads = pc.BATCH[::9]
    ids = [f"read{i}" for i in range(len(reads))]
    eng.upload(reads)
    eng.run()
    before, rec, gt = eng.report_bytes(ids), eng.fetch(), eng.genotype_loci(pc.TEXTS, 3)
    pg = eng.genotype_partial(pc.TEXTS, 3)
    assert int(pg.partial.sum()) >= 30
    assert eng.report_bytes(ids) == before and len(before) > 0
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    assert all(torch.equal(a, b) for a, b in zip(eng.genotype_loci(pc.TEXTS, 3), gt))
    # before the run: the run's report is a run's without it, and the rows are the same either side of it
    eng.upload(reads)
    first = eng.genotype_partial(pc.TEXTS, 3)
    eng.run()
    assert eng.report_bytes(ids) == before
    assert all(torch.equal(a, b) for a, b in zip(first, pg)) and all(torch.equal(a, b) for a, b in zip(eng.genotype_partial(pc.TEXTS, 3), pg))


def test_reads_to_calls_to_the_evidence_beyond_them(eng):
    """six reads span the 3-base locus with 5 copies, four hold its left flank and run off their end after 20: the call is 5 / 5, and
    partial_support counts four open rows of 20 copies beyond it - on the device's tensors, as they come"""
    rng = np.random.RandomState(77)
    A, M, B = pc.LOCI[2]
    junk = lambda: rng.randint(0, 4, size=int(rng.randint(5, 15))).astype(np.uint8)      # noqa: E731
    reads = [pc.cat(junk(), A, np.tile(M, 5), B, junk()) for _ in range(6)] + [pc.cat(junk(), A, np.tile(M, 20)) for _ in range(4)] + [junk()]
    eng.upload(reads)
    calls = eng.call_alleles(eng.genotype_loci(pc.TEXTS[2:3], 0), min_support=2)
    pg = eng.genotype_partial(pc.TEXTS[2:3], 0)
    _assert_columns(pg, pref.genotype_partial(reads, pc.LOCI[2:3], 0), "spanning and partial reads")
    s = mtr_amd.partial_support(pg, calls)
    assert calls.zygosity.tolist() == [1] and calls.call.tolist() == [[5, 5]]
    assert (s.n_partial.tolist(), s.n_open.tolist(), s.max_copies.tolist(), s.n_beyond.tolist()) == ([4], [4], [20], [4])
    assert s.n_beyond.device == pg.partial.device and mtr_amd.partial_support(pg).n_beyond is None
