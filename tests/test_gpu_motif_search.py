"""Known-motif search on the MI355X (mtr_search_motifs_device, Engine.search_motifs, the kernels of mtr_amd/csrc/motif_search.hip.inc).

Truth is the CPU oracle: wrap_around_DP_sub on the read shifted by one base with rep_start and rep_end lowered by one
(tests/test_motif_search_ref.py holds include/mtr_hip.h's definition to exactly that), the score by the identity
G * matches - MM * mismatches - D * (insertions + deletions), the strand by the definition's rule on the two oracle results.  Every case
demands all eight fields, the score, the ratio and the strand exact."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import motif_search_ref as ref
from tests.oracle_binding import Oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LANE_US = (1, 2, 3, 4, 5, 8, 9, 16)
WAVE_US = (17, 64, 65, 128, 129, 256, 257, 499)
LETTERS = "ACGT"


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


def _text(codes) -> str:
    return "".join(LETTERS[int(c)] for c in codes)


def _motifs(us, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 4, size=u).astype(np.uint8) if k % 2 == 0 else rng.randint(0, 3, size=u).astype(np.uint8) for k, u in enumerate(us)]


def _batch(n, motifs, seed, max_len=300, extra=()):
    """n reads of the four kinds (tests/motif_search_ref.py), read i made for motif i mod m, lengths 1 .. max_len mixed: the first reads pin
    the edges (1, 2, shorter than its motif, max_len), `extra` lengths follow"""
    rng = np.random.RandomState(seed)
    pinned = [1, max_len, 2, 3] + list(extra)
    reads = []
    for i in range(n):
        m = motifs[i % len(motifs)]
        L = pinned[i] if i < len(pinned) else int(rng.randint(1, max_len + 1))
        if i == 6 and n > 6:
            m, L = motifs[-1], max(1, len(motifs[-1]) - 1)                      # a read shorter than the motif it is made of
        reads.append(ref.make_read(rng, ref.KINDS[i % 4], L, m))
    return reads


_WANT = {}


def _want(orc, key, reads, motifs, scores, both=True):
    """the oracle's answer, computed once per (batch, motifs, scores, strands): fields [n, m, 8], score, strand"""
    k = (key, scores, both)
    if k not in _WANT:
        one = ref.oracle_align(orc)
        n, m = len(reads), len(motifs)
        f, s, st = np.zeros((n, m, 8), np.int32), np.zeros((n, m), np.int32), np.zeros((n, m), np.uint8)
        for i, x in enumerate(reads):
            for j, mo in enumerate(motifs):
                got, strand = ref.search(x, mo, *scores, both_strands=both, one=one)
                f[i, j], s[i, j], st[i, j] = got[:8], got[8], strand
        _WANT[k] = (f, s, st)
    return _WANT[k]


def _host(hits):
    return tuple(t.cpu().numpy() for t in hits)


def _assert_hits(hits, want, scores, what=""):
    f, s, r, st = _host(hits)
    wf, ws, wst = want
    assert f.shape == wf.shape and s.shape == ws.shape == r.shape == st.shape
    bad = np.argwhere((f != wf).any(axis=2) | (s != ws) | (st != wst))
    assert len(bad) == 0, (what, len(bad), [(tuple(b), f[tuple(b)].tolist(), int(s[tuple(b)]), int(st[tuple(b)]), wf[tuple(b)].tolist(), int(ws[tuple(b)]),
                                              int(wst[tuple(b)])) for b in bad[:4]])
    G, MM, D = scores
    assert np.array_equal(s, G * f[:, :, 4] - MM * f[:, :, 5] - D * (f[:, :, 6] + f[:, :, 7])), what
    wr = np.where(f[:, :, 2] > 0, f[:, :, 4].astype(np.float32) / np.maximum(f[:, :, 2], 1).astype(np.float32), np.float32(0)).astype(np.float32)
    assert np.array_equal(r, wr), what
    none = s == 0
    assert (f[none] == np.array(ref.NO_HIT, np.int32)).all(), what


def _search(eng, reads, motifs, scores, both=True):
    eng.upload(reads)
    return eng.search_motifs([_text(m) for m in motifs], *scores, both_strands=both)


LANE_MOTIFS = _motifs(LANE_US, 11)


# ---- 1. the lane path at its edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_lane_path_at_its_edges(eng, orc, n):
    """groups of 64 tasks: one read, one short of a group, a full group, one more, two and a partial one; the lanes of a wavefront end on
    different rows; every bucket at both ends of its range; the reference's three score sets"""
    reads = _batch(n, LANE_MOTIFS, 100 + n)
    hit = 0
    for scores in ref.SCORE_SETS:
        want = _want(orc, ("lane", n), reads, LANE_MOTIFS, scores)
        _assert_hits(_search(eng, reads, LANE_MOTIFS, scores), want, scores, f"n {n} scores {scores}")
        hit += int((want[1] > 0).sum())
    assert hit > n * len(LANE_US)


# ---- 2. the wave path --------------------------------------------------------------------------------------------------------------
WAVE_MOTIFS = _motifs(WAVE_US, 12)


def _wave_batch():
    return _batch(65, WAVE_MOTIFS, 200, extra=(1100, 1500))             # two reads cross a 1024-row staging block of dp_forward


@pytest.mark.parametrize("scores", ref.SCORE_SETS)
def test_wave_path(eng, orc, scores):
    """every forward pass dp_wrap chooses among: one column per lane (17, 64), two (65, 128), the whole-wavefront 16-bit pass (129, 256), eight
    chunks (257, 499), the whole read as the window base = -1"""
    reads = _wave_batch()
    assert max(len(x) for x in reads) > 1024
    want = _want(orc, "wave", reads, WAVE_MOTIFS, scores)
    _assert_hits(_search(eng, reads, WAVE_MOTIFS, scores), want, scores, f"scores {scores}")
    assert (want[1] > 0).sum() > 65 * 4


def test_wave_path_with_the_32_bit_passes(eng, orc, monkeypatch):
    """MTR_DP16_MAX_ROWS=0: units of 65 .. 256 bases take dp_forward<2> and <4> instead of the 16-bit passes"""
    monkeypatch.setenv("MTR_DP16_MAX_ROWS", "0")
    reads, scores = _wave_batch(), ref.SCORE_SETS[0]
    _assert_hits(_search(eng, reads, WAVE_MOTIFS, scores), _want(orc, "wave", reads, WAVE_MOTIFS, scores), scores)


# ---- 3. the two paths agree ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 130])
def test_the_two_paths_agree(eng, orc, monkeypatch, n):
    reads, scores = _batch(n, LANE_MOTIFS, 100 + n), ref.SCORE_SETS[1]
    by_lanes = _host(_search(eng, reads, LANE_MOTIFS, scores))
    monkeypatch.setenv("MTR_TEST_MOTIF_LANE_MAX", "0")
    waves = _search(eng, reads, LANE_MOTIFS, scores)
    for a, b in zip(by_lanes, _host(waves)):
        assert np.array_equal(a, b)
    _assert_hits(waves, _want(orc, ("lane", n), reads, LANE_MOTIFS, scores), scores)


def test_the_largest_bucket_when_asked_for(eng, orc, monkeypatch):
    """MTR_TEST_MOTIF_LANE_MAX=32: motifs of 17 .. 32 bases take the lane path's 32-column instantiation"""
    monkeypatch.setenv("MTR_TEST_MOTIF_LANE_MAX", "32")
    motifs, scores = _motifs((17, 31, 32, 16), 13), ref.SCORE_SETS[0]
    reads = _batch(70, motifs, 250)
    _assert_hits(_search(eng, reads, motifs, scores), _want(orc, "bucket32", reads, motifs, scores), scores)


# ---- 4. reads either side of the lane path's row bound in one call ---------------------------------------------------------------------
def test_lane_rows_bound_splits_a_call_between_the_kernels(eng, orc, monkeypatch):
    monkeypatch.setenv("MTR_TEST_MOTIF_LANE_ROWS", "100")
    reads, scores = _batch(130, LANE_MOTIFS, 230), ref.SCORE_SETS[2]
    rng = np.random.RandomState(231)
    reads[10] = ref.make_read(rng, "tandem", 100, LANE_MOTIFS[2])             # a read of exactly the bound: the lane path's longest
    reads[11] = ref.make_read(rng, "tandem", 101, LANE_MOTIFS[2])             # and one just beyond it
    lens = np.array([len(x) for x in reads])
    assert (lens > 100).sum() > 20 and (lens <= 100).sum() > 20
    _assert_hits(_search(eng, reads, LANE_MOTIFS, scores), _want(orc, "rows100", reads, LANE_MOTIFS, scores), scores)


# ---- 5. strands ---------------------------------------------------------------------------------------------------------------------
def test_strands(eng, orc):
    rng = np.random.RandomState(5)
    motifs = [ref.codes_of(s) for s in ("CAG", "GGGGCC", "AT", "ACGT", "AACCCT", "ACAC")]
    reads = [ref.make_read(rng, "tandem", 90 + 7 * k, ref.revcomp(m)) for k, m in enumerate(motifs)]      # read k: the other strand of motif k
    reads += [ref.make_read(rng, "tandem", 120, m) for m in motifs]                                       # and the motif's own
    scores = (1, 1, 1)
    want = _want(orc, "strands", reads, motifs, scores)
    hits = _search(eng, reads, motifs, scores)
    _assert_hits(hits, want, scores)
    f, s, _, st = _host(hits)
    one = ref.oracle_align(orc)
    for k in (0, 1, 4):                                                                                   # no palindromes: the other strand wins
        assert st[k, k] == 1 and tuple(f[k, k]) + (int(s[k, k]),) == one(reads[k], ref.revcomp(motifs[k]), *scores)
        assert st[len(motifs) + k, k] == 0
    assert (st[:, 2] == 0).all() and (st[:, 3] == 0).all()                                                # AT and ACGT are their own reverse complement
    assert s[2, 2] > 40 and s[3, 3] > 40
    assert f[len(motifs) + 5, 5, 3] in range(22, 34)                                                      # ACAC as given: copies of four bases
    fwd = _search(eng, reads, motifs, scores, both=False)
    _assert_hits(fwd, _want(orc, "strands", reads, motifs, scores, both=False), scores)
    assert int(fwd.strand.max()) == 0 and int(fwd.score[0, 0]) < int(s[0, 0])


# ---- 6. protocol --------------------------------------------------------------------------------------------------------------------
def _raw(eng, motifs, scores=(1, 1, 1), both=1, dst=None, off=None):
    data, o = mtr_amd.pack_ids(motifs)
    if off is not None:
        o = np.asarray(off, np.int64)
    nh = C.c_int64(-7)
    st = eng.lib.mtr_search_motifs_device(eng.h, data.ctypes.data, o.ctypes.data, len(o) - 1, *scores, both, dst, C.byref(nh))
    return mtr_amd.STATUS.get(st, st), int(nh.value), eng.lib.mtr_last_error(eng.h).decode()


def _columns(n_hits, dev):
    cols = (torch.full((n_hits * 8,), -77, dtype=torch.int32, device=dev), torch.full((n_hits,), -77, dtype=torch.int32, device=dev),
            torch.full((n_hits,), -77.0, dtype=torch.float32, device=dev), torch.full((n_hits,), 77, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    return cols


def _untouched(cols):
    torch.cuda.synchronize()
    return all(bool((c == (77 if c.dtype == torch.uint8 else -77)).all()) for c in cols)


def test_protocol(eng):
    dev = torch.device("cuda", eng.device)
    reads = _batch(9, LANE_MOTIFS, 300)
    eng.upload(reads)
    assert _raw(eng, ["CAG", "AT"])[:2] == ("MTR_OK", 18)                                            # sizes only
    cols = _columns(18, dev)
    dst = mtr_amd.CMotifHitsDst(*[c.data_ptr() for c in cols], 17)
    st, n, msg = _raw(eng, ["CAG", "AT"], dst=C.byref(dst))
    assert (st, n) == ("MTR_ERR_OVERFLOW", 18) and "17" in msg and _untouched(cols)
    dst = mtr_amd.CMotifHitsDst(cols[0].data_ptr(), cols[1].data_ptr(), None, cols[3].data_ptr(), 18)
    assert _raw(eng, ["CAG", "AT"], dst=C.byref(dst))[0] == "MTR_ERR_BAD_ARG" and _untouched(cols)
    dst = mtr_amd.CMotifHitsDst(*[c.data_ptr() for c in cols], 18)
    for kw, word in ((dict(motifs=[]), "n_motifs"), (dict(motifs=["CAG", ""]), "motif 1"), (dict(motifs=["A" * 500]), "motif 0"),
                     (dict(motifs=["CAG", "CAg"]), "motif 1"), (dict(motifs=["CAN"]), "ACGT"), (dict(motifs=["CAG", "AT"], off=[0, 3, 2]), "motif_off"),
                     (dict(motifs=["CAG"], off=[0, 1 << 30]), "2^30"), (dict(motifs=["CAG"], scores=(0, 1, 1)), "gain"), (dict(motifs=["CAG"], scores=(6, 1, 1)), "gain"),
                     (dict(motifs=["CAG"], scores=(1, 0, 1)), "mismatch"), (dict(motifs=["CAG"], scores=(1, 4, 1)), "mismatch"),
                     (dict(motifs=["CAG"], scores=(1, 1, 0)), "indel"), (dict(motifs=["CAG"], scores=(1, 1, 4)), "indel")):
        st, _, msg = _raw(eng, dst=C.byref(dst), **kw)
        assert st == "MTR_ERR_BAD_ARG" and word in msg, (kw, st, msg)
    assert _untouched(cols)
    assert _raw(eng, ["A" * 499])[:2] == ("MTR_OK", 9)                                               # the longest motif there is
    st, n, _ = _raw(eng, ["CAG", "AT"], dst=C.byref(dst))
    assert (st, n) == ("MTR_OK", 18) and not _untouched(cols)


def test_no_batch_and_too_many_hits():
    e = mtr_amd.Engine()
    try:
        st, _, msg = _raw(e, ["CAG"])
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
        n = 46500                                                                                    # n reads x n motifs: beyond 2^31 - 1 hits
        e.upload([np.zeros(1, np.uint8)] * n)
        st, _, msg = _raw(e, ["A"] * n)
        assert st == "MTR_ERR_BAD_ARG" and "2^31" in msg, msg
        assert _raw(e, ["A"] * 3)[:2] == ("MTR_OK", 3 * n)
    finally:
        e.close()


def test_dp_too_large_is_decided_before_any_launch(monkeypatch):
    """under a lowered WrapDPsize (read by mtr_create): (U + 1) * L + U reaches it for the 300-base read and the 64-base motif alone"""
    dev = torch.device("cuda", 0)
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(65 * 300 + 64))
    e = mtr_amd.Engine()
    try:
        rng = np.random.RandomState(8)
        reads = [rng.randint(0, 4, size=L).astype(np.uint8) for L in (100, 299, 300, 300, 50)]
        e.upload(reads)
        motifs = ["CAG", _text(rng.randint(0, 4, size=63)), _text(rng.randint(0, 4, size=64))]
        cols = _columns(15, dev)
        dst = mtr_amd.CMotifHitsDst(*[c.data_ptr() for c in cols], 15)
        st, _, msg = _raw(e, motifs, dst=C.byref(dst))
        assert st == "MTR_ERR_DP_TOO_LARGE" and "read 2" in msg and "motif 2" in msg and _untouched(cols), msg
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_DP_TOO_LARGE"):
            e.search_motifs(motifs)
        hits = e.search_motifs(motifs[:2])                                                           # one base less: fits
        assert hits.score.shape == (5, 2)
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                                                                     # the device's limit back to the built-in one


# ---- 7. nothing else moves ---------------------------------------------------------------------------------------------------------
def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_search_leaves_the_run_and_its_reports_alone(eng):
    reads = [c for _, c in synth.make_reads("c2", 12, 9)] + [np.tile(np.array([1, 0, 2], np.uint8), 70)]
    motifs = ["CAG", "TTAGGG", _text(np.random.RandomState(3).randint(0, 4, size=70))]
    eng.upload(reads)
    eng.run()
    rep, mot, rec = eng.report_tensors(), eng.report_motif_tensors(), eng.fetch()
    assert len(rep.read) > 0
    hits = eng.search_motifs(motifs)
    assert int(hits.score[-1, 0]) >= 200 and int(hits.fields[-1, 0, 3]) >= 68
    assert _same(eng.report_tensors(), rep) and _same(eng.report_motif_tensors(), mot)
    again = eng.fetch()
    assert [[tuple(r) for r in rd] for rd in again] == [[tuple(r) for r in rd] for rd in rec]
    # the search before the run: the run's records are a run's without it
    eng.upload(reads)
    first = eng.search_motifs(motifs)
    eng.run()
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    assert _same(first, hits) and _same(eng.search_motifs(motifs), hits)


def test_file_order_mode_gives_the_same_hits(eng):
    reads = _batch(20, LANE_MOTIFS, 400)
    motifs = [_text(m) for m in LANE_MOTIFS] + ["A" * 70]
    eng.upload(reads)
    plain = eng.search_motifs(motifs)
    fs = mtr_amd.FileState()
    eng.upload(reads, file_state=fs)
    assert _same(eng.search_motifs(motifs), plain)
