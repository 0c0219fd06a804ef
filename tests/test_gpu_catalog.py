"""The catalogue genotype on the MI355X (mtr_genotype_catalog_device, mtr_genotype_catalog_copy_device, Engine.genotype_catalog, the kernels of
mtr_amd/csrc/catalog.hip.inc).  Truth for the rows is the dense call, Engine.genotype_loci, on the same reads and loci: the sparse rows must be
its rows with spanning = 1, in its order, every column bit for bit.  Truth for the candidate count is tests/catalog_ref.py.  The cases are
tests/catalog_cases.py's, which tests/test_catalog_ref.py shows not to be degenerate."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import catalog_cases as cc
from tests import catalog_ref as cref
from tests import flank_ref as fref
from tests.test_gpu_genotype import PATH_IDS, PATHS

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _texts(loci):
    return [tuple(fref.text(s) for s in locus) for locus in loci]


def _assert_rows_of(sg, dense, what=""):
    """sg is dense's spanning rows: (read, locus) the sorted index of spanning == 1, every column torch.equal to the dense row"""
    at = torch.nonzero(dense.spanning == 1)
    assert sg.read.dtype == torch.int32 and sg.locus.dtype == torch.int32
    assert torch.equal(sg.read.long(), at[:, 0]) and torch.equal(sg.locus.long(), at[:, 1]), (what, sg.read.numel(), at.shape[0])
    for name, s, d in zip(mtr_amd.Genotypes._fields, sg[4:11], dense):
        want = d[at[:, 0], at[:, 1]]
        assert s.dtype == want.dtype and s.shape == want.shape and torch.equal(s, want), (what, name)


@pytest.mark.parametrize("K,q", cc.KQ)
def test_the_rows_are_the_dense_call_s_on_every_arrangement_and_both_words(eng, monkeypatch, K, q):
    loci, reads = cc.cases(K, q)
    want_candidates = len(cref.candidates(reads, loci, K, q))
    eng.upload(reads)
    texts = _texts(loci)
    dense = eng.genotype_loci(texts, K)
    assert int(dense.spanning.sum()) >= 35
    first = None
    for word in (None, "64"):
        if word:
            monkeypatch.setenv("MTR_TEST_FLANK_WORD", word)
        for path, name in zip(PATHS, PATH_IDS):
            if path:
                monkeypatch.setenv(*path)
            sg = eng.genotype_catalog(texts, K, q)
            if path:
                monkeypatch.delenv(path[0])
            _assert_rows_of(sg, dense, f"K = {K}, q = {q}, {name}, word {word}")
            assert sg.candidates == want_candidates and (sg.n_reads, sg.n_loci) == (len(reads), len(loci))
            first = first or sg
            assert all(torch.equal(a, b) for a, b in zip(first[2:11], sg[2:11])), name
        if word:
            monkeypatch.delenv("MTR_TEST_FLANK_WORD")
    assert all(torch.equal(a, b) for a, b in zip(first.to_dense(), dense))
    ids, lens = [f"r{i}" for i in range(len(reads))], [len(r) for r in reads]
    assert mtr_amd.format_sparse_genotypes(ids, lens, texts, first) == mtr_amd.format_genotypes(ids, lens, texts, dense)
    if (K + 1) * q <= 32:                                                              # the default seed length is the largest the flanks admit
        assert mtr_amd.pick_seed_len(texts, K) == min(16, min(min(len(a), len(b)) for a, _, b in texts) // (K + 1))
        _assert_rows_of(eng.genotype_catalog(texts, K), dense, "seed_len = None")


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257])
def test_counts_either_side_of_a_wavefront_and_a_workgroup(eng, count):
    """reads[:count] has exactly `count` candidates and `count` rows; two reads without a seed go in front so that the batch is never empty"""
    loci, reads = cc.count_cases(257)
    blank = [np.zeros(50, np.uint8), np.zeros(3, np.uint8)]
    eng.upload(blank + reads[:count])
    sg = eng.genotype_catalog(_texts(loci), 2, 12)
    assert sg.candidates == count and sg.read.numel() == count and sg.read.tolist() == list(range(2, count + 2))
    _assert_rows_of(sg, eng.genotype_loci(_texts(loci), 2), str(count))


def test_a_catalogue_the_dense_call_cannot_take_in_one_piece(eng):
    A, motifs, B, reads, carried = cc.big_catalog()
    K, q = cc.BIG_K, cc.BIG_Q
    letters = np.frombuffer(b"ACGT", np.uint8)
    flank = lambda F: [bytes(row) for row in letters[F]]      # noqa: E731
    loci = list(zip(flank(A), [bytes(letters[m]) for m in motifs], flank(B)))
    eng.upload(reads)
    sg = eng.genotype_catalog(loci, K, q)
    others = [l for l in range(0, cc.BIG_LOCI, cc.BIG_LOCI // 20) if l not in carried][:20]
    sub = sorted(carried + others)
    dense = eng.genotype_loci([loci[l] for l in sub], K)
    assert int(dense.spanning.sum()) == len(reads) and sg.n_loci == cc.BIG_LOCI
    mapped = mtr_amd.SparseGenotypes(sg.n_reads, len(sub), sg.read, torch.tensor([sub.index(l) for l in sg.locus.tolist()], dtype=torch.int32, device=sg.locus.device), *sg[4:])
    _assert_rows_of(mapped, dense, "100 000 loci")
    assert sg.candidates == len(reads)


# ---- protocol ---------------------------------------------------------------------------------------------------------------------------
def _raw(eng, loci, K=1, q=8, scores=(1, 1, 1)):
    data, o = mtr_amd.pack_ids([s for locus in loci for s in locus])
    nr, nc = C.c_int64(-7), C.c_int64(-7)
    st = eng.lib.mtr_genotype_catalog_device(eng.h, data.ctypes.data, o.ctypes.data, len(loci), K, q, *scores, C.byref(nr), C.byref(nc))
    return mtr_amd.STATUS.get(st, st), int(nr.value), int(nc.value), eng.lib.mtr_last_error(eng.h).decode()


def _copy(eng, cols, cap):
    dst = mtr_amd.CCatalogDst(cols[0].data_ptr(), cols[1].data_ptr(), mtr_amd.CGenotypesDst(*[t.data_ptr() for t in cols[2:]], cap))
    st = eng.lib.mtr_genotype_catalog_copy_device(eng.h, C.byref(dst))
    return mtr_amd.STATUS.get(st, st)


def _columns(eng, R, fill=77):
    dev = torch.device("cuda", eng.device)
    shapes = ((R, torch.int32), (R, torch.int32), (R, torch.uint8), (R, torch.uint8), (2 * R, torch.int32), (2 * R, torch.int32), (8 * R, torch.int32), (R, torch.int32),
              (R, torch.float32))
    cols = [torch.full((n,), fill, dtype=t, device=dev) for n, t in shapes]
    torch.cuda.synchronize()
    return cols


def test_the_copy_protocol_and_the_argument_errors():
    loci, reads = cc.cases(1, 8)
    texts = _texts(loci)
    e = mtr_amd.Engine()
    try:
        e.upload(reads)
        cols = _columns(e, 4)
        assert _copy(e, cols, 4) == "MTR_ERR_BAD_ARG" and "comes first" in e.lib.mtr_last_error(e.h).decode()      # nothing kept yet
        st, R, Cn, _ = _raw(e, texts)
        assert st == "MTR_OK" and R >= 40 and Cn >= R
        cols = _columns(e, R)
        assert _copy(e, cols, R - 1) == "MTR_ERR_OVERFLOW"
        dst = mtr_amd.CCatalogDst(cols[0].data_ptr(), None, mtr_amd.CGenotypesDst(*[t.data_ptr() for t in cols[2:]], R))
        assert mtr_amd.STATUS[e.lib.mtr_genotype_catalog_copy_device(e.h, C.byref(dst))] == "MTR_ERR_BAD_ARG"
        torch.cuda.synchronize()
        assert all(bool((c == 77).all()) for c in cols)
        assert _copy(e, cols, R) == "MTR_OK" and int(cols[2].min()) == 1 and int(cols[0].max()) < len(reads)
        ok = ("ACGTACGTACGGTCAT", "CAG", "TTGACCGATAGGCTAA")
        for kw, word in ((dict(q=7), "seed_len"), (dict(q=17), "seed_len"), (dict(loci=[ok, (ok[0], "CAG", ok[2][:15])]), "locus 1, right flank"),
                         (dict(loci=[(ok[0][:15], "CAG", ok[2])]), "locus 0, left flank"), (dict(K=2), "locus 0, left flank"), (dict(K=-1), "max_flank_dist"),
                         (dict(q=7, scores=(0, 1, 1)), "gain"), (dict(loci=[]), "n_loci")):
            st, R2, Cn2, msg = _raw(e, **{"loci": [ok], **kw})
            assert st == "MTR_ERR_BAD_ARG" and word in msg and (R2, Cn2) == (0, 0), (kw, st, msg)
        assert _copy(e, cols, R) == "MTR_ERR_BAD_ARG"                                      # a failed call keeps nothing
        with pytest.raises(mtr_amd.MtrError, match="fewer than 8"):
            e.genotype_catalog([ok], 2)
        with pytest.raises(mtr_amd.MtrError):
            e.genotype_catalog([ok[:2]], 1)
        _assert_rows_of(e.genotype_catalog(texts, 1, 8), e.genotype_loci(texts, 1), "after the errors")
        e.upload(reads[:3])
        assert _copy(e, cols, R) == "MTR_ERR_BAD_ARG"                                      # an upload discards what was kept
    finally:
        e.close()


def test_dp_too_large_comes_where_the_dense_call_gives_it(monkeypatch):
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(65 * 300 + 64))
    e = mtr_amd.Engine()
    try:
        rng = np.random.RandomState(8)
        e.upload([rng.randint(0, 4, size=L).astype(np.uint8) for L in (100, 299, 300, 50)])
        t = lambda n: fref.text(rng.randint(0, 4, size=n))      # noqa: E731
        loci = [(t(20), "CAG", t(20)), (t(20), t(63), t(20)), (t(20), t(64), t(20))]
        def dense(loci, K=1):
            data, o = mtr_amd.pack_ids([s for locus in loci for s in locus])
            nr = C.c_int64()
            st = e.lib.mtr_genotype_loci_device(e.h, data.ctypes.data, o.ctypes.data, len(loci), K, 1, 1, 1, None, C.byref(nr))
            return mtr_amd.STATUS.get(st, st), e.lib.mtr_last_error(e.h).decode()

        st, _, _, msg = _raw(e, loci)
        assert st == "MTR_ERR_DP_TOO_LARGE" and "read 2" in msg and "motif 2" in msg, msg
        assert (st, msg) == dense(loci)                                                   # the dense call's verdict and its words
        for sub in (loci[:1], loci[:2], loci[1:], loci[2:]):
            assert _raw(e, sub)[0] == dense(sub)[0], sub
        assert _raw(e, loci, K=-1)[0] == dense(loci, K=-1)[0] == "MTR_ERR_BAD_ARG"
        assert _raw(e, loci, K=-1)[0] == "MTR_ERR_BAD_ARG"                                # the genotype's arguments come before it
        assert _raw(e, loci, q=7)[0] == "MTR_ERR_DP_TOO_LARGE"                            # the new checks after it
        assert _raw(e, loci[:2])[0] == "MTR_OK"
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                                                         # the device's limit back to the built-in one


def test_a_catalogue_call_leaves_the_run_and_the_kept_loci_alone(eng):
    loci, reads = cc.cases(1, 8)
    texts = _texts(loci)
    eng.upload(reads[:40])
    eng.run()
    motifs = [texts[1][1], texts[5][1]]
    rec, kept = eng.fetch(), eng.search_motif_loci(motifs, 6)
    sg = eng.genotype_catalog(texts, 1, 8)
    assert sg.read.numel() >= 20
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    dev = torch.device("cuda", eng.device)
    P, T = kept.loci_off.numel() - 1, kept.fields.shape[0]
    off, fields = torch.empty(P + 1, dtype=torch.int64, device=dev), torch.empty((T, 8), dtype=torch.int32, device=dev)
    rest = [torch.empty(T, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.float32, device=dev), torch.empty(T, dtype=torch.uint8, device=dev),
            torch.empty(P, dtype=torch.uint8, device=dev)]
    torch.cuda.synchronize()
    dst = mtr_amd.CMotifLociDst(off.data_ptr(), fields.data_ptr(), *[t.data_ptr() for t in rest], P, T)
    assert mtr_amd.STATUS[eng.lib.mtr_motif_loci_copy_device(eng.h, C.byref(dst))] == "MTR_OK"                 # ml_ready survives
    assert torch.equal(off, kept.loci_off) and torch.equal(fields, kept.fields)
