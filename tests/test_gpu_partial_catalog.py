"""The partial genotype at catalogue scale on the MI355X (mtr_genotype_partial_catalog_device, mtr_genotype_partial_catalog_copy_device,
Engine.genotype_partial_catalog, the kernels of mtr_amd/csrc/partial_catalog.hip.inc).  Truth for the rows is the dense call,
Engine.genotype_partial, on the same reads and loci - tests/test_gpu_partial.py holds that call to the Python definition -: the sparse rows must
be its rows with partial = 1, in its order, every column torch.equal.  Truth for the candidate count is tests/partial_catalog_ref.py.  The cases
are tests/partial_catalog_cases.py's, which tests/test_partial_catalog_ref.py shows not to be degenerate."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import catalog_cases as cc
from tests import flank_ref as fref
from tests import partial_cases as pc
from tests import partial_catalog_cases as pcc
from tests import partial_catalog_ref as pcr

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _texts(loci):
    return [tuple(fref.text(s) for s in locus) for locus in loci]


def _assert_rows_of(spg, dense, what=""):
    """spg is dense's partial rows: (read, locus) the sorted index of partial == 1, every column torch.equal to the dense row"""
    at = torch.nonzero(dense.partial == 1)
    assert spg.read.dtype == torch.int32 and spg.locus.dtype == torch.int32
    assert torch.equal(spg.read.long(), at[:, 0]) and torch.equal(spg.locus.long(), at[:, 1]), (what, spg.read.numel(), at.shape[0])
    for name, s, d in zip(mtr_amd.PartialGenotypes._fields, spg[4:11], dense):
        want = d[at[:, 0], at[:, 1]]
        assert s.dtype == want.dtype and s.shape == want.shape, (what, name, s.shape, want.shape)
        if not torch.equal(s, want):
            i = int(torch.nonzero((s != want).reshape(s.shape[0], -1).any(dim=1))[0])
            raise AssertionError((what, name, i, int(spg.read[i]), int(spg.locus[i]), s[i].tolist(), want[i].tolist()))
    assert bool((spg.partial == 1).all())


def _both_words_and_scores(eng, monkeypatch, loci, reads, K, q):
    texts = _texts(loci)
    want_candidates = len(pcr.candidates(reads, loci, K, q))
    eng.upload(reads)
    for scores in ((1, 1, 1), (2, 3, 2)):
        dense = eng.genotype_partial(texts, K, *scores, max_tail=pcc.MAX_TAIL)
        first = None
        for word in (None, "64"):
            if word:
                monkeypatch.setenv("MTR_TEST_FLANK_WORD", word)
            spg = eng.genotype_partial_catalog(texts, K, q, *scores, max_tail=pcc.MAX_TAIL)
            if word:
                monkeypatch.delenv("MTR_TEST_FLANK_WORD")
            _assert_rows_of(spg, dense, f"K = {K}, q = {q}, {scores}, word {word}")
            assert spg.candidates == want_candidates and (spg.n_reads, spg.n_loci) == (len(reads), len(loci))
            key = spg.read.long() * len(loci) + spg.locus.long()
            assert bool((key[1:] > key[:-1]).all())                                        # sorted by (read, locus), no pair twice
            first = first or spg
            assert all(torch.equal(a, b) for a, b in zip(first[2:11], spg[2:11]))
        assert all(torch.equal(a, b) for a, b in zip(first.to_dense(), dense))
    return texts, dense, first


@pytest.mark.parametrize("K,q", pcc.GRID_KQ)
def test_the_grid_s_rows_are_the_dense_call_s(eng, monkeypatch, K, q):
    texts, dense, spg = _both_words_and_scores(eng, monkeypatch, pc.LOCI, pc.BATCH, K, q)
    assert spg.candidates == pcc.GRID_COUNTS[(K, q)][0]
    ids, lens = [f"r{i}" for i in range(len(pc.BATCH))], [len(r) for r in pc.BATCH]
    assert mtr_amd.format_sparse_partial_genotypes(ids, lens, texts, spg) == mtr_amd.format_partial_genotypes(ids, lens, texts, dense)
    if (K + 1) * q <= 20:                                                                  # the default seed length is the largest the flanks admit
        _assert_rows_of(eng.genotype_partial_catalog(texts, K, None, 2, 3, 2, max_tail=pcc.MAX_TAIL), dense, "seed_len = None")


@pytest.mark.parametrize("K,q", pcc.KQ)
def test_the_new_set_s_rows_are_the_dense_call_s(eng, monkeypatch, K, q):
    loci, reads = pcc.cases(K, q)
    _, dense, _ = _both_words_and_scores(eng, monkeypatch, loci, reads, K, q)
    assert int(dense.partial.sum()) >= 200


def test_max_tail_moves_open_and_nothing_else(eng):
    loci, reads = pcc.cases(3, 8)
    texts = _texts(loci)
    eng.upload(reads)
    base = eng.genotype_partial_catalog(texts, 3, 8, max_tail=10)
    seen = set()
    for max_tail in (0, 10):
        spg = eng.genotype_partial_catalog(texts, 3, 8, max_tail=max_tail)
        assert all(torch.equal(a, b) for a, b in zip(spg[2:10], base[2:10])), max_tail
        assert torch.equal(spg.open, (spg.ext[:, 5] <= max_tail).to(torch.uint8))
        seen.add(int(spg.open.sum()))
    assert len(seen) == 2


@pytest.mark.parametrize("first_u,last_u,n", [(5, 8, 130), (17, 32, 70)])
def test_every_lane_runs_its_own_motif_length_and_direction(eng, first_u, last_u, n):
    """one launch of one bucket, n tasks of n loci in all four slots: 64 consecutive tasks are 64 motifs of four lengths (sixteen in the bucket
    of 32) in both directions.  An extension kernel that took the motif, its length or the direction from lane 0 would be right for at most the
    lanes that share lane 0's - tests/test_partial_catalog_ref.py shows that no two loci share a motif and that consecutive reads differ in
    length and direction"""
    loci, reads, what = pcc.mixed(first_u, last_u, n)
    texts = _texts(loci)
    eng.upload(reads)
    dense = eng.genotype_partial(texts, 0, max_tail=pcc.MAX_TAIL)
    spg = eng.genotype_partial_catalog(texts, 0, 12, max_tail=pcc.MAX_TAIL)
    assert spg.read.tolist() == list(range(n)) and spg.locus.tolist() == list(range(n)) and spg.slot.tolist() == [s for _, s, _ in what]
    assert (spg.window[:, 1] - spg.window[:, 0]).tolist() == [wl for _, _, wl in what] and bool((spg.ext[:, 0] > 0).all())
    _assert_rows_of(spg, dense, f"motifs of {first_u} .. {last_u} bases")
    assert spg.candidates == len(pcr.candidates(reads, loci, 0, 12))


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_counts_either_side_of_a_wavefront_and_a_workgroup(eng, count):
    """reads[:count] has exactly `count` candidates, rows and tasks; two reads without a seed go in front so that the batch is never empty"""
    loci, reads = pcc.count_cases(257)
    texts = _texts(loci)
    blank = [np.zeros(50, np.uint8), np.zeros(3, np.uint8)]
    eng.upload(blank + reads[:count])
    spg = eng.genotype_partial_catalog(texts, 2, 12, max_tail=pcc.MAX_TAIL)
    assert spg.candidates == count and spg.read.tolist() == list(range(2, count + 2))
    _assert_rows_of(spg, eng.genotype_partial(texts, 2, max_tail=pcc.MAX_TAIL), str(count))
    if count == 0:
        assert all(t.numel() == 0 for t in spg[2:11]) and spg.ext.shape == (0, 6) and spg.window.shape == (0, 2)
        dst = mtr_amd.CPartialCatalogDst(None, None, mtr_amd.CPartialDst(None, None, None, None, None, None, None, 0))
        assert mtr_amd.STATUS[eng.lib.mtr_genotype_partial_catalog_copy_device(eng.h, C.byref(dst))] == "MTR_OK"      # nothing to write: NULL columns pass


def test_a_catalogue_the_dense_call_cannot_take_in_one_piece(eng):
    A, motifs, B, reads, carried = pcc.big_cut()
    K, q = cc.BIG_K, cc.BIG_Q
    letters = np.frombuffer(b"ACGT", np.uint8)
    flank = lambda F: [bytes(row) for row in letters[F]]      # noqa: E731
    loci = list(zip(flank(A), [bytes(letters[m]) for m in motifs], flank(B)))
    eng.upload(reads)
    spg = eng.genotype_partial_catalog(loci, K, q)
    others = [l for l in range(0, cc.BIG_LOCI, cc.BIG_LOCI // 20) if l not in carried][:20]
    sub = sorted(carried + others)
    dense = eng.genotype_partial([loci[l] for l in sub], K)
    assert int(dense.partial.sum()) == len(reads) and spg.n_loci == cc.BIG_LOCI
    assert set(spg.locus.tolist()) == set(carried)                                         # no row of a locus that is not carried
    mapped = mtr_amd.SparsePartialGenotypes(spg.n_reads, len(sub), spg.read, torch.tensor([sub.index(l) for l in spg.locus.tolist()], dtype=torch.int32, device=spg.locus.device),
                                            *spg[4:])
    _assert_rows_of(mapped, dense, "100 000 loci")
    assert spg.candidates == len(pcr.candidates(reads, [(A[l], motifs[l], B[l]) for l in carried], K, q))      # (the other loci have no seed in any read)


# ---- protocol ---------------------------------------------------------------------------------------------------------------------------
def _raw(eng, loci, K=1, q=8, scores=(1, 1, 1), max_tail=10, off=None):
    data, o = mtr_amd.pack_ids([s for locus in loci for s in locus])
    if off is not None:
        o = np.array(off, np.int64)
    nr, nc = C.c_int64(-7), C.c_int64(-7)
    st = eng.lib.mtr_genotype_partial_catalog_device(eng.h, data.ctypes.data, o.ctypes.data, len(loci), K, q, *scores, max_tail, C.byref(nr), C.byref(nc))
    return mtr_amd.STATUS.get(st, st), int(nr.value), int(nc.value), eng.lib.mtr_last_error(eng.h).decode()


def _columns(eng, R, fill=77):
    dev = torch.device("cuda", eng.device)
    shapes = ((R, torch.int32), (R, torch.int32), (R, torch.uint8), (R, torch.uint8), (R, torch.int32), (2 * R, torch.int32), (6 * R, torch.int32), (R, torch.float32),
              (R, torch.uint8))
    cols = [torch.full((n,), fill, dtype=t, device=dev) for n, t in shapes]
    torch.cuda.synchronize()
    return cols


def _copy(eng, cols, cap, null=None):
    ptrs = [None if k == null else c.data_ptr() for k, c in enumerate(cols)]
    dst = mtr_amd.CPartialCatalogDst(ptrs[0], ptrs[1], mtr_amd.CPartialDst(*ptrs[2:], cap))
    st = eng.lib.mtr_genotype_partial_catalog_copy_device(eng.h, C.byref(dst))
    return mtr_amd.STATUS.get(st, st)


def _catalog_copy(eng, R):
    dev = torch.device("cuda", eng.device)
    new = lambda dtype, *tail: torch.empty((R,) + tail, dtype=dtype, device=dev)     # noqa: E731
    cols = (new(torch.int32), new(torch.int32), new(torch.uint8), new(torch.uint8), new(torch.int32, 2), new(torch.int32, 2), new(torch.int32, 8), new(torch.int32), new(torch.float32))
    torch.cuda.synchronize()
    dst = mtr_amd.CCatalogDst(cols[0].data_ptr(), cols[1].data_ptr(), mtr_amd.CGenotypesDst(*[t.data_ptr() for t in cols[2:]], R))
    st = eng.lib.mtr_genotype_catalog_copy_device(eng.h, C.byref(dst))
    return mtr_amd.STATUS.get(st, st), cols


def test_the_copy_protocol_the_kept_rows_and_the_argument_errors():
    loci, reads = pcc.cases(3, 8)
    texts = _texts(loci)
    e = mtr_amd.Engine()
    try:
        e.upload(reads)
        cols = _columns(e, 4)
        assert _copy(e, cols, 4) == "MTR_ERR_BAD_ARG" and "comes first" in e.lib.mtr_last_error(e.h).decode()      # nothing kept yet
        assert mtr_amd.STATUS[e.lib.mtr_genotype_partial_catalog_copy_device(e.h, None)] == "MTR_ERR_BAD_ARG"
        st, R, Cn, _ = _raw(e, texts, K=3)
        assert st == "MTR_OK" and R >= 200 and Cn > R
        assert mtr_amd.STATUS[e.lib.mtr_genotype_partial_catalog_copy_device(e.h, None)] == "MTR_ERR_BAD_ARG"
        cols = _columns(e, R)
        assert _copy(e, cols, R - 1) == "MTR_ERR_OVERFLOW"
        for k in range(9):
            assert _copy(e, cols, R, null=k) == "MTR_ERR_BAD_ARG", k
        torch.cuda.synchronize()
        assert all(bool((c == 77).all()) for c in cols)
        assert _copy(e, cols, R) == "MTR_OK" and int(cols[2].min()) == 1 and int(cols[0].max()) < len(reads)
        # two calls give byte-identical columns
        assert _raw(e, texts, K=3)[:3] == ("MTR_OK", R, Cn)
        again = _columns(e, R, fill=55)
        assert _copy(e, again, R) == "MTR_OK" and all(torch.equal(a, b) for a, b in zip(cols, again))
        # the catalogue genotype's kept rows survive this call, and this call's survive that one: both copied afterwards, both correct
        sg = e.genotype_catalog(texts, 3, 8)
        assert sg.read.numel() >= 16
        assert _raw(e, texts, K=3)[:3] == ("MTR_OK", R, Cn)
        e.genotype_catalog(texts, 3, 8)
        st, kept = _catalog_copy(e, sg.read.numel())
        assert st == "MTR_OK" and all(torch.equal(a.reshape(b.shape), b) for a, b in zip(kept, sg[2:11]))
        third = _columns(e, R, fill=33)
        assert _copy(e, third, R) == "MTR_OK" and all(torch.equal(a, b) for a, b in zip(cols, third))
        dense = e.genotype_partial(texts, 3)
        spg = mtr_amd.SparsePartialGenotypes(len(reads), len(loci), third[0], third[1], third[2], third[3], third[4], third[5].reshape(R, 2), third[6].reshape(R, 6),
                                             third[7], third[8], Cn)
        _assert_rows_of(spg, dense, "copied after a catalogue call")
        st, kept = _catalog_copy(e, sg.read.numel())                                       # the dense partial call discards neither
        assert st == "MTR_OK"
        # each argument error, in the stated order; the batch stays usable and nothing is kept after a failed call
        ok = ("ACGTACGTACGGTCAT", "CAG", "TTGACCGATAGGCTAA")
        big = (ok[0], "A" * 33, ok[2])
        for kw, word in ((dict(loci=[]), "n_loci"), (dict(off=[0, 16, 15, 35]), "decreases"), (dict(scores=(0, 1, 1)), "gain"), (dict(scores=(5, 4, 7)), "mismatch"),
                         (dict(loci=[ok, (ok[0], "", ok[2])]), "motif 1"), (dict(loci=[ok, ("", "CAG", ok[2])]), "locus 1, left flank"), (dict(K=-1), "max_flank_dist"),
                         (dict(loci=[big], K=-1), "max_flank_dist"), (dict(loci=[ok, big], max_tail=-1, q=7), "locus 1"), (dict(max_tail=-1, q=7), "max_tail"),
                         (dict(loci=[(ok[0][:15], "CAG", ok[2])], q=17), "seed_len"), (dict(q=7), "seed_len"), (dict(q=17), "seed_len"),
                         (dict(loci=[ok, (ok[0], "CAG", ok[2][:15])]), "locus 1, right flank"), (dict(loci=[(ok[0][:15], "CAG", ok[2])]), "locus 0, left flank"),
                         (dict(K=2), "locus 0, left flank")):
            st, R2, Cn2, msg = _raw(e, **{"loci": [ok], **kw})
            assert st == "MTR_ERR_BAD_ARG" and word in msg and (R2, Cn2) == (0, 0), (kw, st, msg)
            assert _copy(e, cols, R) == "MTR_ERR_BAD_ARG"                                  # a failed call keeps nothing
        assert _raw(e, [ok, (ok[0], "A" * 32, ok[2])])[0] == "MTR_OK"                      # 32 bases are taken
        st, kept = _catalog_copy(e, sg.read.numel())                                       # the failed calls did not touch the other call's rows
        assert st == "MTR_OK" and all(torch.equal(a.reshape(b.shape), b) for a, b in zip(kept, sg[2:11]))
        with pytest.raises(mtr_amd.MtrError, match="fewer than 8"):
            e.genotype_partial_catalog([ok], 2)
        with pytest.raises(mtr_amd.MtrError):
            e.genotype_partial_catalog([ok[:2]], 1)
        _assert_rows_of(e.genotype_partial_catalog(texts, 3, 8), dense, "after the errors")
        e.upload(reads[:3])
        assert _copy(e, cols, R) == "MTR_ERR_BAD_ARG"                                      # an upload discards what was kept
    finally:
        e.close()


def test_no_batch():
    e = mtr_amd.Engine()
    try:
        st, _, _, msg = _raw(e, [("ACGTACGTACGGTCAT", "CAG", "TTGACCGATAGGCTAA")])
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
        st, _, _, msg = _raw(e, [], K=-1)                                                  # the batch is asked for first
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
    finally:
        e.close()


def test_no_dp_too_large(monkeypatch):
    """under a WrapDPsize at which the genotype refuses the batch this call answers: it stores no cell"""
    loci, reads = pcc.cases(3, 8)
    texts = _texts(loci)
    longest = max(len(r) for r in reads)
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(33 * (longest - 5)))                     # the longest read against the 32-base motif does not fit
    e = mtr_amd.Engine()
    try:
        e.upload(reads)
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
            e.genotype_catalog(texts, 3, 8)
        _assert_rows_of(e.genotype_partial_catalog(texts, 3, 8), e.genotype_partial(texts, 3), "a small WrapDPsize")
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                                                           # the device's limit back to the built-in one


def test_the_call_leaves_the_run_and_its_report_alone(eng):
    loci, reads = pcc.cases(3, 8)
    texts = _texts(loci)
    reads = reads[::3]
    ids = [f"read{i}" for i in range(len(reads))]
    eng.upload(reads)
    eng.run()
    before, rec = eng.report_bytes(ids), eng.fetch()
    spg = eng.genotype_partial_catalog(texts, 3, 8)
    _assert_rows_of(spg, eng.genotype_partial(texts, 3), "after a run")
    assert spg.read.numel() >= len(reads) // 2                                             # (two reads in three of the set hold a single flank)
    assert eng.report_bytes(ids) == before and len(before) > 0
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    eng.upload(reads)
    first = eng.genotype_partial_catalog(texts, 3, 8)
    eng.run()
    assert eng.report_bytes(ids) == before
    assert all(torch.equal(a, b) for a, b in zip(first[2:11], spg[2:11])) and all(torch.equal(a, b) for a, b in zip(eng.genotype_partial_catalog(texts, 3, 8)[2:11], spg[2:11]))


def test_reads_to_calls_to_the_evidence_beyond_them(eng):
    """six reads span the 3-base locus with 5 copies, four hold its left flank and run off their end after 20: the call is 5 / 5 from the catalogue
    genotype's sparse rows, and partial_support counts four open rows of 20 copies beyond it from this call's sparse rows - as from the dense ones"""
    rng = np.random.RandomState(77)
    A, M, B = pc.LOCI[2]
    other = pc.TEXTS[5]
    junk = lambda: rng.randint(0, 4, size=int(rng.randint(5, 15))).astype(np.uint8)      # noqa: E731
    reads = [pc.cat(junk(), A, np.tile(M, 5), B, junk()) for _ in range(6)] + [pc.cat(junk(), A, np.tile(M, 20)) for _ in range(4)] + [junk()]
    texts = [other, pc.TEXTS[2]]
    eng.upload(reads)
    calls = eng.call_alleles(eng.genotype_catalog(texts, 0, 16), min_support=2)
    spg = eng.genotype_partial_catalog(texts, 0, 16)
    pg = eng.genotype_partial(texts, 0)
    _assert_rows_of(spg, pg, "spanning and partial reads")
    s, d = mtr_amd.partial_support(spg, calls), mtr_amd.partial_support(pg, calls)
    assert calls.zygosity.tolist()[1] == 1 and calls.call.tolist()[1] == [5, 5]
    assert (s.n_partial.tolist(), s.n_open.tolist(), s.max_copies.tolist(), s.n_beyond.tolist()) == ([0, 4], [0, 4], [0, 20], [0, 4])
    assert all(torch.equal(a, b) and a.dtype == b.dtype and a.device == b.device for a, b in zip(s, d))
    assert mtr_amd.partial_support(spg).n_beyond is None and all(torch.equal(a, b) for a, b in zip(mtr_amd.partial_support(spg)[:3], mtr_amd.partial_support(pg)[:3]))
