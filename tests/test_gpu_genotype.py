"""Locus genotyping on the MI355X (mtr_genotype_loci_device, Engine.genotype_loci, the kernels of mtr_amd/csrc/genotype.hip.inc over those of
flank_search.hip.inc and motif_loci.hip.inc).

Truth for the pairing is tests/flank_ref.py (the flank hits as a full edit-distance matrix, then the rules of include/mtr_hip.h); truth for the
alignment is the CPU oracle on the sliced read, as tests/test_gpu_motif_search.py takes it.  Every column must be exact for K = 0 and K = 3 on
every arrangement of the alignment's two paths (tests/test_gpu_motif_loci.py's: the default border, no lane path, the largest bucket, a row
bound of 100), with equal columns across the arrangements.  Reads are random + A~ + (M x c)~ + B~ + random on both strands for c = 0, 1, 2, 5
and 30 - or, for the motifs of 16 bases and more, as many copies as keep a read within 400 bases."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import flank_ref as fref
from tests import motif_search_ref as ref
from tests.oracle_binding import Oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

PATHS = [None, ("MTR_TEST_MOTIF_LANE_MAX", "0"), ("MTR_TEST_MOTIF_LANE_MAX", "32"), ("MTR_TEST_MOTIF_LANE_ROWS", "100")]
PATH_IDS = ["default", "lane_max_0", "lane_max_32", "lane_rows_100"]
COPIES = (0, 1, 2, 5, 30)


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    o = Oracle()
    yield o
    o.close()


def _loci():
    """motifs of 1, 3, 6 and 16 bases (the lane path by default) and of 17 and 40 (the wave path); flanks of 12 .. 64 bases"""
    rng = np.random.RandomState(41)
    out = []
    for U, fl in zip((1, 3, 6, 16, 17, 40), ((20, 24), (12, 33), (64, 20), (32, 32), (25, 63), (31, 18))):
        M = rng.randint(0, 4, size=U).astype(np.uint8)
        while U > 1 and len(set(M.tolist())) == 1:
            M = rng.randint(0, 4, size=U).astype(np.uint8)
        out.append((rng.randint(0, 4, size=fl[0]).astype(np.uint8), M, rng.randint(0, 4, size=fl[1]).astype(np.uint8)))
    return out


LOCI = _loci()


def _edited(rng, p, edits):
    q = [int(v) for v in p]
    for _ in range(edits):
        at, what = int(rng.randint(0, len(q))), int(rng.randint(0, 3))
        if what == 0:
            q[at] = (q[at] + 1 + int(rng.randint(0, 3))) & 3
        elif what == 1 and len(q) > 1:
            del q[at]
        else:
            q.insert(at, int(rng.randint(0, 4)))
    return np.array(q, np.uint8)


def _cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts]).astype(np.uint8)


def _batch():
    rng = np.random.RandomState(42)
    junk = lambda lo, hi: rng.randint(0, 4, size=int(rng.randint(lo, hi + 1))).astype(np.uint8)      # noqa: E731
    reads = []
    for A, M, B in LOCI:
        U = len(M)
        for c in COPIES:
            c = min(c, 280 // U)
            for noisy in (0, 1):                                                   # clean flanks (they span at K = 0), then one or two edits each
                for strand in (0, 1):
                    rep = np.tile(M, c)
                    rep = _edited(rng, rep, (c * U) // 25 if noisy else 0) if c else rep
                    x = _cat(junk(0, 12), _edited(rng, A, noisy * (1 + len(reads) % 2)), rep, _edited(rng, B, noisy * (1 + (len(reads) // 2) % 2)), junk(0, 12))
                    reads.append(ref.revcomp(x) if strand else x)
    A, M, B = LOCI[1]
    A3, M3, B3 = LOCI[3]
    five = np.tile(M, 5)
    reads += [
        _cat(junk(5, 20), A, five, junk(30, 40)),                                  # the right flank is missing
        _cat(junk(30, 40), five, B, junk(5, 20)),                                  # the left one
        ref.revcomp(_cat(junk(5, 20), A, five, junk(30, 40))),
        _cat(five, B, junk(5, 20)),                                                # the read begins inside the repeat
        ref.revcomp(_cat(five[1:], B, junk(5, 20))),
        _cat(junk(0, 9), B, five, A, junk(0, 9)),                                  # the flanks in the wrong order
        ref.revcomp(_cat(B, five, A)),
        _cat(A, five, B, junk(20, 30), ref.revcomp(_cat(A, np.tile(M, 2), B))),    # both orientations valid, a tie: orientation 0
        _cat(_edited(rng, A, 1), five, B, junk(20, 30), ref.revcomp(_cat(A, np.tile(M, 2), B))),      # the reverse one is nearer (K = 3)
        _cat(A3, M3[:7], B3),                                                      # a window shorter than its motif
        ref.revcomp(_cat(junk(3, 9), A3, M3[:15], B3)),
        _cat(A, B), _cat(B3), np.zeros(1, np.uint8),                               # an allele of no copies; one flank and nothing else; one base
    ]
    assert max(len(r) for r in reads) <= 400
    return reads


BATCH = _batch()
_WANT = {}


def _want(orc, K, scores=(1, 1, 1)):
    if (K, scores) not in _WANT:
        _WANT[(K, scores)] = fref.genotype(BATCH, LOCI, K, *scores, one=ref.oracle_align(orc))
    return _WANT[(K, scores)]


def _texts():
    return [tuple(fref.text(s) for s in locus) for locus in LOCI]


def _assert_columns(gt, want, what=""):
    for name, g, w in zip(mtr_amd.Genotypes._fields, (t.cpu().numpy() for t in gt), want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            r, k = int(at[0]), int(at[1])
            raise AssertionError((what, name, r, k, g[r, k].tolist(), w[r, k].tolist(), [c[r, k].tolist() for c in want]))


def test_the_batch_is_not_degenerate(orc):
    """from the reference alone: enough spanning pairs in each orientation, an empty window, a window shorter than its motif, and a pair of
    each kind that does not span"""
    U = np.array([len(M) for _, M, _ in LOCI])
    for K in (0, 3):
        (sp, o, fd, w, f, sc, _), why = _want(orc, K)
        assert ((sp == 1) & (o == 0)).sum() >= 20 and ((sp == 1) & (o == 1)).sum() >= 20, (K, int(sp.sum()))
        length = w[:, :, 1] - w[:, :, 0]
        assert ((sp == 1) & (length == 0)).sum() >= 1 and ((sp == 1) & (length > 0) & (length < U[None, :])).sum() >= 1
        assert {"left", "right", "order"} <= {kind for _, _, kind in why}, sorted({kind for _, _, kind in why})
        assert f[:, :, 3].max() >= 30 and ((sp == 1) & (f[:, :, 3] == 1)).sum() >= 2 and (fd.max() > 0) == (K > 0)
    # the two reads with both orientations valid: the tie is orientation 0; with K = 3 the nearer pair of flanks wins
    both = len(BATCH) - 6
    (sp, o, fd, *_), _ = _want(orc, 3)
    assert (sp[both - 1, 1], o[both - 1, 1], sp[both, 1], o[both, 1]) == (1, 0, 1, 1) and fd[both, 1].tolist() == [0, 0]
    (sp, o, *_), _ = _want(orc, 0)
    assert (sp[both, 1], o[both, 1]) == (1, 1)


@pytest.mark.parametrize("K", [0, 3])
def test_every_column_on_every_arrangement_of_the_paths(eng, orc, monkeypatch, K):
    want, _ = _want(orc, K)
    eng.upload(BATCH)
    first = None
    for path, name in zip(PATHS, PATH_IDS):
        if path:
            monkeypatch.setenv(*path)
        gt = eng.genotype_loci(_texts(), K)
        if path:
            monkeypatch.delenv(path[0])
        _assert_columns(gt, want, f"K = {K}, {name}")
        first = first or gt
        assert all(torch.equal(a, b) for a, b in zip(first, gt)), name
    ids, lens = [f"r{i}" for i in range(len(BATCH))], [len(r) for r in BATCH]
    text = mtr_amd.format_genotypes(ids, lens, _texts(), first)
    assert text == mtr_amd.format_genotypes(ids, lens, _texts(), mtr_amd.Genotypes(*want)) and text.count(b"\n") == int(want[0].sum())


def test_other_scores_and_the_same_call_twice(eng, orc):
    scores = ref.SCORE_SETS[0]
    want, _ = _want(orc, 3, scores)
    eng.upload(BATCH)
    gt = eng.genotype_loci(_texts(), 3, *scores)
    _assert_columns(gt, want, str(scores))
    again = eng.genotype_loci(_texts(), 3, *scores)
    assert all(torch.equal(a, b) for a, b in zip(gt, again))
    assert not np.array_equal(want[5], _want(orc, 3)[0][5])


def test_one_locus_one_read(eng, orc):
    A, M, B = LOCI[2]
    read = _cat(A, np.tile(M, 4), B)
    eng.upload([read])
    gt = eng.genotype_loci([tuple(fref.text(s) for s in LOCI[2])], 0)
    assert gt.spanning.shape == (1, 1) and gt.window.cpu().tolist() == [[[64, 88]]]
    assert gt.fields.cpu().tolist() == [[[64, 87, 24, 4, 24, 0, 0, 0]]] and gt.score.item() == 24 and gt.ratio.item() == 1.0


# ---- protocol ---------------------------------------------------------------------------------------------------------------------------
def _raw(eng, loci, K=2, scores=(1, 1, 1), off=None):
    flat = [s for locus in loci for s in locus]
    data, o = mtr_amd.pack_ids(flat)
    if off is not None:
        o = np.array(off, np.int64)
    nr = C.c_int64(-7)
    st = eng.lib.mtr_genotype_loci_device(eng.h, data.ctypes.data, o.ctypes.data, len(loci), K, *scores, None, C.byref(nr))
    return mtr_amd.STATUS.get(st, st), int(nr.value), eng.lib.mtr_last_error(eng.h).decode()


def test_the_argument_errors_and_the_batch_stays_usable(eng, orc):
    eng.upload(BATCH)
    ok = ("ACGTACGTAC", "CAG", "TTGACCGATA")
    for kw, word in ((dict(loci=[]), "n_loci"), (dict(loci=[ok], off=[0, 10, 9, 20]), "decreases"), (dict(loci=[ok], scores=(0, 1, 1)), "gain"),
                     (dict(loci=[ok], scores=(1, 4, 1)), "mismatch"), (dict(loci=[ok], scores=(1, 1, 0)), "indel"), (dict(loci=[ok, ("ACGT", "", "ACGT")]), "motif 1"),
                     (dict(loci=[("ACGT", "A" * 500, "ACGT")]), "motif 0"), (dict(loci=[("ACGT", "CAN", "ACGT")]), "ACGT"), (dict(loci=[ok, ("", "CAG", "ACGT")]), "locus 1, left flank"),
                     (dict(loci=[("ACGT", "CAG", "A" * 65)]), "right flank"), (dict(loci=[("ACGU", "CAG", "ACGT")]), "left flank"), (dict(loci=[ok], K=-1), "max_flank_dist"),
                     (dict(loci=[("", "CAG", "ACGT")], K=-1), "left flank"), (dict(loci=[ok], K=-1, scores=(9, 1, 1)), "gain")):
        st, R, msg = _raw(eng, **kw)
        assert st == "MTR_ERR_BAD_ARG" and word in msg and R == 0, (kw, st, msg)
    assert _raw(eng, [ok, ("A" * 64, "C" * 499, "G")])[:2] == ("MTR_OK", 2 * len(BATCH))
    with pytest.raises(mtr_amd.MtrError):
        eng.genotype_loci([("ACGT", "CAG")], 1)
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
        eng.genotype_loci([ok], -2)
    # a destination too small, and a NULL column: nothing written
    dev = torch.device("cuda", eng.device)
    R = len(BATCH)
    shapes = ((R, torch.uint8), (R, torch.uint8), (2 * R, torch.int32), (2 * R, torch.int32), (8 * R, torch.int32), (R, torch.int32), (R, torch.float32))
    cols = [torch.full((n,), 77, dtype=t, device=dev) for n, t in shapes]
    torch.cuda.synchronize()
    data, o = mtr_amd.pack_ids(list(ok))
    nr = C.c_int64()
    call = lambda dst: mtr_amd.STATUS[eng.lib.mtr_genotype_loci_device(eng.h, data.ctypes.data, o.ctypes.data, 1, 2, 1, 1, 1, C.byref(dst), C.byref(nr))]      # noqa: E731
    ptrs = [c.data_ptr() for c in cols]
    assert call(mtr_amd.CGenotypesDst(*ptrs, R - 1)) == "MTR_ERR_OVERFLOW"
    assert call(mtr_amd.CGenotypesDst(*ptrs[:4], None, *ptrs[5:], R)) == "MTR_ERR_BAD_ARG"
    torch.cuda.synchronize()
    assert all(bool((c == 77).all()) for c in cols)
    assert call(mtr_amd.CGenotypesDst(*ptrs, R)) == "MTR_OK" and int(nr.value) == R and int(cols[0].max()) <= 1
    _assert_columns(eng.genotype_loci(_texts(), 3), _want(orc, 3)[0], "after the errors")


def test_no_batch():
    e = mtr_amd.Engine()
    try:
        st, _, msg = _raw(e, [("ACGT", "CAG", "ACGT")])
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
        st, _, msg = _raw(e, [], K=-1)                                                                 # the batch is asked for first
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
    finally:
        e.close()


def test_dp_too_large_is_decided_from_the_whole_reads(monkeypatch):
    """under a lowered WrapDPsize (read by mtr_create): the 300-base read and the 64-base motif alone reach it, whatever the window would be"""
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(65 * 300 + 64))
    e = mtr_amd.Engine()
    try:
        rng = np.random.RandomState(8)
        e.upload([rng.randint(0, 4, size=L).astype(np.uint8) for L in (100, 299, 300, 50)])
        t = lambda n: fref.text(rng.randint(0, 4, size=n))      # noqa: E731
        loci = [(t(20), "CAG", t(20)), (t(20), t(63), t(20)), (t(20), t(64), t(20))]
        st, _, msg = _raw(e, loci)
        assert st == "MTR_ERR_DP_TOO_LARGE" and "read 2" in msg and "motif 2" in msg, msg
        assert _raw(e, loci, K=-1)[0] == "MTR_ERR_BAD_ARG"                                            # the arguments come before it
        assert e.genotype_loci(loci[:2], 2).spanning.shape == (4, 2)
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                                                                     # the device's limit back to the built-in one


# ---- nothing else moves -------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_genotype_leaves_the_run_the_reports_and_the_kept_loci_alone(eng):
    eng.upload(BATCH[:40])
    eng.run()
    motifs = [fref.text(LOCI[1][1]), fref.text(LOCI[5][1])]
    rep, rec, hits, loci = eng.report_tensors(), eng.fetch(), eng.search_motifs(motifs), eng.search_motif_loci(motifs, 6)
    gt = eng.genotype_loci(_texts(), 3)
    assert int(gt.spanning.sum()) >= 30
    assert _same(eng.report_tensors(), rep) and _same(eng.search_motifs(motifs), hits)
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    # what the locus search kept is still there to be copied
    dev = torch.device("cuda", eng.device)
    P, T = loci.loci_off.numel() - 1, loci.fields.shape[0]
    off, fields = torch.empty(P + 1, dtype=torch.int64, device=dev), torch.empty((T, 8), dtype=torch.int32, device=dev)
    rest = [torch.empty(T, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.float32, device=dev), torch.empty(T, dtype=torch.uint8, device=dev),
            torch.empty(P, dtype=torch.uint8, device=dev)]
    torch.cuda.synchronize()
    dst = mtr_amd.CMotifLociDst(off.data_ptr(), fields.data_ptr(), *[t.data_ptr() for t in rest], P, T)
    assert mtr_amd.STATUS[eng.lib.mtr_motif_loci_copy_device(eng.h, C.byref(dst))] == "MTR_OK"
    assert torch.equal(off, loci.loci_off) and torch.equal(fields, loci.fields) and torch.equal(rest[0], loci.score)
    # the genotype before the run: the run's records are a run's without it, and the rows are the same either side of it
    eng.upload(BATCH[:40])
    first = eng.genotype_loci(_texts(), 3)
    eng.run()
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    assert _same(first, gt) and _same(eng.genotype_loci(_texts(), 3), gt)
