"""Known-motif locus search on the MI355X (mtr_search_motif_loci_device, mtr_motif_loci_copy_device, Engine.search_motif_loci, the kernels of
mtr_amd/csrc/motif_loci.hip.inc).

Truth is tests/motif_loci_ref.py - the recursion of include/mtr_hip.h in Python - over the CPU oracle as aligner, as tests/test_gpu_motif_search.py
takes it (tests/test_motif_loci_ref.py holds that recursion to the plain-Python aligner).  Every case demands loci_off, all eight fields, the score,
the ratio, the strand and the open flags exact, and every case runs on every arrangement of the two paths: the default border, no lane path at all
(MTR_TEST_MOTIF_LANE_MAX=0), the largest bucket (=32), and a row bound of 100 (MTR_TEST_MOTIF_LANE_ROWS), which sends the long reads through the
wave path and their short children through the lanes in one call."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import motif_loci_ref as lref
from tests import motif_search_ref as ref
from tests.oracle_binding import Oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LETTERS = "ACGT"
PATHS = [None, ("MTR_TEST_MOTIF_LANE_MAX", "0"), ("MTR_TEST_MOTIF_LANE_MAX", "32"), ("MTR_TEST_MOTIF_LANE_ROWS", "100")]
PATH_IDS = ["default", "lane_max_0", "lane_max_32", "lane_rows_100"]


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


@pytest.fixture(params=PATHS, ids=PATH_IDS)
def path(request, monkeypatch):
    if request.param:
        monkeypatch.setenv(*request.param)
    return request.param


def _text(codes) -> str:
    return "".join(LETTERS[int(c)] for c in codes)


# ---- the batches ---------------------------------------------------------------------------------------------------------------------
def _motifs():
    """1, 4, 5, 16, 17 and 33 bases - the buckets' edges, the lane / wave border, the wave path - and the palindrome AT"""
    rng = np.random.RandomState(21)
    return [rng.randint(0, 4 if k % 2 else 3, size=u).astype(np.uint8) for k, u in enumerate((1, 4, 5, 16, 17, 33))] + [ref.codes_of("AT")]


MOTIFS = _motifs()


def _main_batch():
    """70 reads - a full group of 64 and a partial one - of lengths 1 .. 600, the four kinds in turn, read i made for motif i mod 7"""
    rng = np.random.RandomState(22)
    pinned = [1, 600, 2, 3, 599, 101, 100]
    return [ref.make_read(rng, ref.KINDS[i % 4], pinned[i] if i < len(pinned) else int(rng.randint(1, 601)), MOTIFS[i % len(MOTIFS)]) for i in range(70)]


MAIN = _main_batch()


def _staircase():
    """runs of A of 24, 23 .. 9 bases between 25 C each: under motif A every run is a locus, the longest is the leftmost, so the recursion goes
    down the right side only, sixteen levels deep"""
    parts = []
    for k in range(24, 8, -1):
        parts += [np.zeros(k, np.uint8), np.full(25, 1, np.uint8)]
    return np.concatenate(parts[:-1])


def _crafted():
    cag = ref.codes_of("CAG")
    edges = np.concatenate([np.tile(cag, 10), np.zeros(15, np.uint8), np.full(16, 3, np.uint8), np.tile(cag, 7)])      # tracts on base 0 and on base L - 1
    return [lref.three_tracts(), edges, np.zeros(600, np.uint8), _staircase()]


CRAFTED, CRAFTED_MOTIFS = _crafted(), [ref.codes_of("CAG"), ref.codes_of("A")]

_WANT = {}


def _want(orc, key, reads, motifs, scores, S, R, both=True):
    """the reference's columns, computed once per case"""
    k = (key, scores, S, R, both)
    if k not in _WANT:
        _WANT[k] = lref.columns(reads, motifs, *scores, S, R, both, one=ref.oracle_align(orc))
    return _WANT[k]


def _host(loci):
    return tuple(t.cpu().numpy() for t in loci)


def _assert_loci(loci, want, what=""):
    got = _host(loci)
    for name, g, w in zip(mtr_amd.MotifLoci._fields, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
    off, woff = got[0], want[0]
    bad = np.flatnonzero(off != woff)
    assert len(bad) == 0, (what, "loci_off", [(int(p), int(off[p]), int(woff[p])) for p in bad[:4]])
    for name, g, w in list(zip(mtr_amd.MotifLoci._fields, got, want))[1:]:
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError((what, name, at.tolist(), g[tuple(at[:1])].tolist(), w[tuple(at[:1])].tolist()))


def _search(eng, reads, motifs, scores, S, R, both=True):
    eng.upload(reads)
    return eng.search_motif_loci([_text(m) for m in motifs], S, *scores, both_strands=both, max_rounds=R)


# ---- 1. the smallest shapes that can still go wrong, on every arrangement of the paths -------------------------------------------------
@pytest.mark.parametrize("both", [True, False], ids=["both_strands", "forward"])
@pytest.mark.parametrize("scores", ref.SCORE_SETS)
def test_every_locus_of_the_main_batch(eng, orc, path, scores, both):
    S = 6 * scores[0]
    want = _want(orc, "main", MAIN, MOTIFS, scores, S, 16, both)
    _assert_loci(_search(eng, MAIN, MOTIFS, scores, S, 16, both), want, f"{path} {scores} {both}")
    per_pair = np.diff(want[0])
    # two_runs and more: several loci per pair (a gain of 5 bridges most junk: few there)
    assert want[0][-1] > 150 and (per_pair >= 2).sum() >= (3 if scores[0] == 5 else 100), (int(want[0][-1]), int((per_pair >= 2).sum()))
    if both:
        assert want[4].sum() > 5 and (want[4][np.repeat(np.arange(len(per_pair)) % len(MOTIFS) == 6, per_pair)] == 0).all()      # AT is its own reverse complement


def test_the_crafted_reads(eng, orc, path):
    """the three-tract read (strands 0, 1, 0), tracts on the read's first and last base, poly-A under motif A (one locus: the whole read - the
    recursion's children are empty), and the staircase of A runs: sixteen loci, one level each, down the right side"""
    scores = (1, 1, 1)
    want = _want(orc, "crafted", CRAFTED, CRAFTED_MOTIFS, scores, 8, 32)
    loci = _search(eng, CRAFTED, CRAFTED_MOTIFS, scores, 8, 32)
    _assert_loci(loci, want, str(path))
    off, f, s, _, st, op = _host(loci)
    three = slice(off[0], off[1])
    assert st[three][s[three] >= 18].tolist() == [0, 1, 0]
    edges = f[off[2]:off[3]]
    assert edges[0, 0] == 0 and edges[-1, 1] == len(CRAFTED[1]) - 1 and len(edges) >= 2
    assert off[6] - off[5] == 1 and f[off[5]].tolist() == [0, 599, 600, 600, 600, 0, 0, 0] and s[off[5]] == 600
    stairs = f[off[7]:off[8]]
    assert stairs[:, 2].tolist() == list(range(24, 8, -1)) and not op.any()


def test_too_few_rounds_leave_the_pair_open(eng, orc, path):
    want = _want(orc, "crafted", CRAFTED, CRAFTED_MOTIFS, (1, 1, 1), 8, 3)
    loci = _search(eng, CRAFTED, CRAFTED_MOTIFS, (1, 1, 1), 8, 3)
    _assert_loci(loci, want, str(path))
    off, f, _, _, _, op = _host(loci)
    assert op[3, 1] == 1 and op[2, 1] == 0 and f[off[7]:off[8], 2].tolist() == [24, 23, 22]            # the staircase: three levels, and more to find


# ---- 2. one round is the search ---------------------------------------------------------------------------------------------------------
def test_one_round_is_search_motifs_where_the_score_reaches_the_threshold(eng, path):
    scores, S = ref.SCORE_SETS[0], 40
    text = [_text(m) for m in MOTIFS]
    eng.upload(MAIN)
    hits = eng.search_motifs(text, *scores)
    loci = eng.search_motif_loci(text, S, *scores, max_rounds=1)
    keep = (hits.score >= S).reshape(-1)
    assert 50 < int(keep.sum()) < keep.numel()
    assert torch.equal(loci.loci_off, torch.cat([torch.zeros(1, dtype=torch.int64, device=keep.device), torch.cumsum(keep.to(torch.int64), 0)]))
    assert torch.equal(loci.fields, hits.fields.reshape(-1, 8)[keep]) and torch.equal(loci.score, hits.score.reshape(-1)[keep])
    assert torch.equal(loci.ratio, hits.ratio.reshape(-1)[keep]) and torch.equal(loci.strand, hits.strand.reshape(-1)[keep])
    assert loci.open.shape == hits.score.shape and int(loci.open.sum()) > 0 and not bool(loci.open.reshape(-1)[~keep].any())


# ---- 3. the same call twice -------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes(eng, path):
    scores, S = ref.SCORE_SETS[2], 6
    first = _search(eng, MAIN + CRAFTED, MOTIFS, scores, S, 16)
    again = eng.search_motif_loci([_text(m) for m in MOTIFS], S, *scores, max_rounds=16)
    third = _search(eng, MAIN + CRAFTED, MOTIFS, scores, S, 16)
    assert int(first.loci_off[-1]) > 300
    for a, b, c in zip(first, again, third):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---- 4. protocol ------------------------------------------------------------------------------------------------------------------------
def _raw(eng, motifs, scores=(1, 1, 1), both=1, S=5, R=16):
    data, o = mtr_amd.pack_ids(motifs)
    npairs, nloci = C.c_int64(-7), C.c_int64(-7)
    st = eng.lib.mtr_search_motif_loci_device(eng.h, data.ctypes.data, o.ctypes.data, len(o) - 1, *scores, both, S, R, C.byref(npairs), C.byref(nloci))
    return mtr_amd.STATUS.get(st, st), int(npairs.value), int(nloci.value), eng.lib.mtr_last_error(eng.h).decode()


def _columns(P, T, dev):
    cols = (torch.full((P + 1,), -77, dtype=torch.int64, device=dev), torch.full((max(T, 1) * 8,), -77, dtype=torch.int32, device=dev),
            torch.full((max(T, 1),), -77, dtype=torch.int32, device=dev), torch.full((max(T, 1),), -77.0, dtype=torch.float32, device=dev),
            torch.full((max(T, 1),), 77, dtype=torch.uint8, device=dev), torch.full((P,), 77, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    return cols


def _untouched(cols):
    torch.cuda.synchronize()
    return all(bool((c == (77 if c.dtype == torch.uint8 else -77)).all()) for c in cols)


def _copy(eng, cols, P, T):
    dst = mtr_amd.CMotifLociDst(*[c.data_ptr() if c is not None else None for c in cols], P, T)
    st = eng.lib.mtr_motif_loci_copy_device(eng.h, C.byref(dst))
    return mtr_amd.STATUS.get(st, st), eng.lib.mtr_last_error(eng.h).decode()


def test_protocol(eng):
    dev = torch.device("cuda", eng.device)
    eng.upload(CRAFTED)
    st, P, T, _ = _raw(eng, ["CAG", "A"], S=8)
    assert (st, P) == ("MTR_OK", 8) and T >= 3 + 2 + 1 + 16
    cols = _columns(P, T, dev)
    assert _copy(eng, cols, P, T - 1)[0] == "MTR_ERR_OVERFLOW" and _untouched(cols)
    st, msg = _copy(eng, cols, P - 1, T)
    assert st == "MTR_ERR_OVERFLOW" and str(P - 1) in msg and _untouched(cols)
    assert _copy(eng, cols[:3] + (None,) + cols[4:], P, T)[0] == "MTR_ERR_BAD_ARG" and _untouched(cols)
    assert _copy(eng, (None,) + cols[1:], P, T)[0] == "MTR_ERR_BAD_ARG" and _untouched(cols)
    assert eng.lib.mtr_motif_loci_copy_device(eng.h, None) == [k for k, v in mtr_amd.STATUS.items() if v == "MTR_ERR_BAD_ARG"][0]
    assert _copy(eng, cols, P, T)[0] == "MTR_OK" and not _untouched(cols)
    assert int(cols[0][-1]) == T and _copy(eng, _columns(P + 3, T + 5, dev), P + 3, T + 5)[0] == "MTR_OK"       # the copy may be repeated, into more room
    # the arguments: the search's checks in the search's order, then the two of this call
    for kw, word in ((dict(motifs=[]), "n_motifs"), (dict(motifs=["CAG", ""]), "motif 1"), (dict(motifs=["CAN"]), "ACGT"), (dict(motifs=["CAG"], scores=(0, 1, 1)), "gain"),
                     (dict(motifs=["CAG"], scores=(1, 4, 1)), "mismatch"), (dict(motifs=["CAG"], scores=(1, 1, 0)), "indel"),
                     (dict(motifs=["CAG"], S=0), "min_score"), (dict(motifs=["CAG"], S=-3), "min_score"), (dict(motifs=["CAG"], R=0), "max_rounds"),
                     (dict(motifs=["CAG"], R=33), "max_rounds"), (dict(motifs=["CAG"], scores=(0, 1, 1), S=0), "gain"), (dict(motifs=["CAG"], S=0, R=0), "min_score")):
        st, P2, T2, msg = _raw(eng, **kw)
        assert st == "MTR_ERR_BAD_ARG" and word in msg and (P2, T2) == (0, 0), (kw, st, msg)
    st, msg = _copy(eng, cols, P, T)                                                                          # a failed search keeps nothing
    assert st == "MTR_ERR_BAD_ARG" and "no loci" in msg
    assert _raw(eng, ["CAG"], R=32)[0] == "MTR_OK" and _raw(eng, ["CAG"], R=1)[0] == "MTR_OK"
    # a search without a locus: offsets and flags alone, NULL columns allowed
    st, P0, T0, _ = _raw(eng, ["GGGGCC"], S=500)
    assert (st, P0, T0) == ("MTR_OK", 4, 0)
    zero = _columns(P0, 0, dev)
    assert _copy(eng, (zero[0], None, None, None, None, zero[5]), P0, 0)[0] == "MTR_OK" and int(zero[0].abs().sum()) == 0 and int(zero[5].sum()) == 0


def test_no_batch_and_an_upload_discards_the_kept_loci():
    e = mtr_amd.Engine()
    try:
        dev = torch.device("cuda", e.device)
        st, _, _, msg = _raw(e, ["CAG"])
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
        st, _, _, msg = _raw(e, ["CAG"], S=0)                                                                # the batch is asked for first
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
        assert _copy(e, _columns(1, 1, dev), 1, 1)[0] == "MTR_ERR_BAD_ARG"
        e.upload(CRAFTED)
        st, P, T, _ = _raw(e, ["CAG"], S=12)
        assert st == "MTR_OK" and T >= 3
        e.run()                                                                                              # a run does not discard them
        cols = _columns(P, T, dev)
        assert _copy(e, cols, P, T)[0] == "MTR_OK" and int(cols[0][-1]) == T
        e.upload(CRAFTED)
        st, msg = _copy(e, _columns(P, T, dev), P, T)
        assert st == "MTR_ERR_BAD_ARG" and "no loci" in msg
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
            e.search_motif_loci(["CAG"], 0)
    finally:
        e.close()


def test_dp_too_large_is_decided_from_the_whole_reads(monkeypatch):
    """under a lowered WrapDPsize (read by mtr_create): the 300-base read and the 64-base motif alone reach it, as in the search's own test"""
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(65 * 300 + 64))
    e = mtr_amd.Engine()
    try:
        rng = np.random.RandomState(8)
        e.upload([rng.randint(0, 4, size=L).astype(np.uint8) for L in (100, 299, 300, 50)])
        motifs = ["CAG", _text(rng.randint(0, 4, size=63)), _text(rng.randint(0, 4, size=64))]
        st, _, _, msg = _raw(e, motifs)
        assert st == "MTR_ERR_DP_TOO_LARGE" and "read 2" in msg and "motif 2" in msg, msg
        assert _raw(e, motifs, S=0)[0] == "MTR_ERR_BAD_ARG"                                                  # the arguments come before it
        assert e.search_motif_loci(motifs[:2], 5).open.shape == (4, 2)
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                                                                             # the device's limit back to the built-in one


# ---- 5. nothing else moves --------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_locus_search_leaves_the_run_its_reports_and_the_search_alone(eng):
    reads = [c for _, c in synth.make_reads("c2", 12, 9)] + [np.tile(np.array([1, 0, 2], np.uint8), 70)]
    motifs = ["CAG", "TTAGGG", _text(np.random.RandomState(3).randint(0, 4, size=70))]
    eng.upload(reads)
    eng.run()
    rep, mot, rec, hits = eng.report_tensors(), eng.report_motif_tensors(), eng.fetch(), eng.search_motifs(motifs)
    assert len(rep.read) > 0
    loci = eng.search_motif_loci(motifs, 10)
    assert int(loci.loci_off[-1]) > 12 and int(loci.score.max()) >= 200
    assert _same(eng.report_tensors(), rep) and _same(eng.report_motif_tensors(), mot) and _same(eng.search_motifs(motifs), hits)
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    # the locus search before the run: the run's records are a run's without it, and the loci are the same either side of it
    eng.upload(reads)
    first = eng.search_motif_loci(motifs, 10)
    eng.run()
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    assert _same(first, loci) and _same(eng.search_motif_loci(motifs, 10), loci) and _same(eng.search_motifs(motifs), hits)
    ids = [f"r{i}" for i in range(len(reads))]
    text = mtr_amd.format_motif_loci(ids, [len(x) for x in reads], motifs, loci, min_copies=0)            # (a locus of a 70-base motif may hold less than one copy)
    assert text.count(b"\n") == int(loci.loci_off[-1]) and text.startswith(b"r0\t")
