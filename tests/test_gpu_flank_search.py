"""Flank search on the MI355X (mtr_search_flanks_device, Engine.search_flanks, the kernels of mtr_amd/csrc/flank_search.hip.inc).

Truth is tests/flank_ref.py - the definition of include/mtr_hip.h as a full edit-distance matrix (tests/test_flank_ref.py holds it to brute
force).  Every column must be exact: as built (patterns of up to 32 bases through the 32-bit scan, longer ones through the 64-bit scan), with
every pattern sent through the 64-bit scan (MTR_TEST_FLANK_WORD=64), and on the forward strand alone."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import flank_ref as fref
from tests import motif_search_ref as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _patterns():
    """1, 2, 20, 31, 32, 33, 63 and 64 bases; the 20-base one is its own reverse complement"""
    rng = np.random.RandomState(31)
    half = rng.randint(0, 4, size=10).astype(np.uint8)
    pats = [rng.randint(0, 4, size=m).astype(np.uint8) for m in (1, 2)] + [np.concatenate([half, ref.revcomp(half)])]
    return pats + [rng.randint(0, 4, size=m).astype(np.uint8) for m in (31, 32, 33, 63, 64)]


PATTERNS = _patterns()
assert [len(p) for p in PATTERNS] == [1, 2, 20, 31, 32, 33, 63, 64] and np.array_equal(ref.revcomp(PATTERNS[2]), PATTERNS[2])


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


def _batch():
    """130 reads of 1 .. 300 bases - two full groups of 64 and a partial one.  Read i of kind i mod 4: 0, 1 = a copy of pattern (i // 4) mod 8 with
    i mod 5 edits planted, as given or reverse-complemented (at the read's very start or end now and then); 2 = random, no planted hit; 3 = a
    read shorter than the long patterns."""
    rng = np.random.RandomState(32)
    pinned = {2: 300, 6: 1, 10: 299, 14: 2}
    reads = []
    for i in range(130):
        L, kind = pinned.get(i, int(rng.randint(1, 301))), i % 4
        if kind >= 2:
            reads.append(rng.randint(0, 4, size=min(L, 40) if kind == 3 else L).astype(np.uint8))
            continue
        q = _edited(rng, PATTERNS[(i // 4) % 8], i % 5)
        q = ref.revcomp(q) if kind == 1 else q
        room = max(0, L - len(q))
        left = 0 if i % 7 == 0 else room if i % 7 == 1 else int(rng.randint(0, room + 1))
        reads.append(np.concatenate([rng.randint(0, 4, size=left), q, rng.randint(0, 4, size=room - left)]).astype(np.uint8))
    return reads


BATCH = _batch()
_WANT = {}


def _want(key, reads, both=True):
    if (key, both) not in _WANT:
        _WANT[(key, both)] = fref.search(reads, PATTERNS, both)
    return _WANT[(key, both)]


def _assert_hits(hits, want, what=""):
    for name, g, w in zip(mtr_amd.FlankHits._fields, (t.cpu().numpy() for t in hits), want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            r, k = np.argwhere(g != w)[0]
            raise AssertionError((what, name, int(r), int(k), int(g[r, k]), int(w[r, k]), [int(c[r, k]) for c in want]))


def _texts():
    return [fref.text(p) for p in PATTERNS]


def test_the_batch_holds_what_it_is_meant_to():
    dist, _, end, strand = _want("batch", BATCH)
    lens = np.array([len(r) for r in BATCH])
    assert len(BATCH) == 130 and lens.min() == 1 and lens.max() == 300
    planted = np.array([dist[i, (i // 4) % 8] for i in range(130) if i % 4 < 2])
    assert set(planted.tolist()) == {0, 1, 2, 3, 4}
    wide = [int(dist[i, (i // 4) % 8]) for i in range(130) if i % 4 < 2 and (i // 4) % 8 >= 5]                  # the patterns of the 64-bit scan
    assert set(wide) == {0, 1, 2, 3, 4}, wide
    assert strand.sum() > 60 and strand[:, 2].sum() == 0                          # both strands win somewhere; the palindrome is always strand 0
    assert (lens[:, None] < np.array([len(p) for p in PATTERNS])[None, :]).sum() > 100
    assert (end == lens[:, None]).sum() > 10 and (dist[:, 7] > 20).sum() > 60        # hits that end on the last base; reads without a planted hit


@pytest.mark.parametrize("word", [None, "64"], ids=["as_built", "word_64"])
@pytest.mark.parametrize("both", [True, False], ids=["both_strands", "forward"])
def test_every_column_of_the_batch(eng, monkeypatch, word, both):
    if word:
        monkeypatch.setenv("MTR_TEST_FLANK_WORD", word)
    eng.upload(BATCH)
    hits = eng.search_flanks(_texts(), both_strands=both)
    _assert_hits(hits, _want("batch", BATCH, both), f"{word} {both}")
    if not both:
        assert int(hits.strand.sum()) == 0


def test_the_two_words_agree(eng, monkeypatch):
    eng.upload(BATCH)
    first = eng.search_flanks(_texts())
    monkeypatch.setenv("MTR_TEST_FLANK_WORD", "64")
    second = eng.search_flanks(_texts())
    monkeypatch.delenv("MTR_TEST_FLANK_WORD")
    third = eng.search_flanks(_texts())
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("word", [None, "64"], ids=["as_built", "word_64"])
def test_a_batch_of_a_single_read(eng, monkeypatch, word):
    if word:
        monkeypatch.setenv("MTR_TEST_FLANK_WORD", word)
    for key, read in (("one", BATCH[0]), ("one_base", BATCH[6])):
        eng.upload([read])
        _assert_hits(eng.search_flanks(_texts()), _want(key, [read]), key)


# ---- protocol ---------------------------------------------------------------------------------------------------------------------------
def _raw(eng, patterns, both=1, off=None):
    data, o = mtr_amd.pack_ids(patterns)
    if off is not None:
        o = np.array(off, np.int64)
    nh = C.c_int64(-7)
    st = eng.lib.mtr_search_flanks_device(eng.h, data.ctypes.data, o.ctypes.data, len(o) - 1, both, None, C.byref(nh))
    return mtr_amd.STATUS.get(st, st), int(nh.value), eng.lib.mtr_last_error(eng.h).decode()


def test_the_argument_errors_and_the_batch_stays_usable(eng):
    eng.upload(BATCH)
    for patterns, off, word in (([], None, "n_patterns"), (["ACG", "TT"], [0, 3, 2], "decreases"), (["ACG", ""], None, "pattern 1"), (["A" * 65], None, "length 65"),
                                (["ACG", "ACN"], None, "ACGT"), (["acg"], None, "ACGT")):
        st, H, msg = _raw(eng, patterns, off=off)
        assert st == "MTR_ERR_BAD_ARG" and word in msg and H == 0, (patterns, st, msg)
    assert _raw(eng, ["A" * 64, "C"])[:2] == ("MTR_OK", 2 * len(BATCH))
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
        eng.search_flanks(["ACGU"])
    with pytest.raises(mtr_amd.MtrError):
        eng.search_flanks("ACG")
    # a destination too small, and a NULL column: nothing written
    dev = torch.device("cuda", eng.device)
    H = 2 * len(BATCH)
    cols = [torch.full((H,), -77, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.full((H,), 77, dtype=torch.uint8, device=dev)]
    torch.cuda.synchronize()
    data, o = mtr_amd.pack_ids(["ACGT", "C"])
    nh = C.c_int64()
    call = lambda dst: mtr_amd.STATUS[eng.lib.mtr_search_flanks_device(eng.h, data.ctypes.data, o.ctypes.data, 2, 1, C.byref(dst), C.byref(nh))]      # noqa: E731
    assert call(mtr_amd.CFlankHitsDst(*[c.data_ptr() for c in cols], H - 1)) == "MTR_ERR_OVERFLOW"
    assert call(mtr_amd.CFlankHitsDst(cols[0].data_ptr(), None, cols[2].data_ptr(), cols[3].data_ptr(), H)) == "MTR_ERR_BAD_ARG"
    torch.cuda.synchronize()
    assert all(bool((c == (77 if c.dtype == torch.uint8 else -77)).all()) for c in cols)
    assert call(mtr_amd.CFlankHitsDst(*[c.data_ptr() for c in cols], H)) == "MTR_OK" and int(nh.value) == H and int(cols[0].min()) >= 0
    _assert_hits(eng.search_flanks(_texts()), _want("batch", BATCH), "after the errors")


def test_no_batch_and_too_many_hits():
    e = mtr_amd.Engine()
    try:
        st, _, msg = _raw(e, ["CAG"])
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
        st, _, msg = _raw(e, [])                                                                     # the batch is asked for first
        assert st == "MTR_ERR_BAD_ARG" and "no batch" in msg
        n = 46500                                                                                    # n reads x n patterns: beyond 2^31 - 1 hits
        e.upload([np.zeros(1, np.uint8)] * n)
        st, _, msg = _raw(e, ["A"] * n)
        assert st == "MTR_ERR_BAD_ARG" and "2^31" in msg, msg
        assert _raw(e, ["A"] * 3)[:2] == ("MTR_OK", 3 * n)
    finally:
        e.close()


# ---- nothing else moves -------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_flank_search_leaves_the_run_and_its_reports_alone(eng):
    reads = [c for _, c in synth.make_reads("c2", 12, 9)] + [np.tile(np.array([1, 0, 2], np.uint8), 70)]
    pats = ["CAGCAGCAGCAG", fref.text(np.random.RandomState(3).randint(0, 4, size=40))]
    eng.upload(reads)
    eng.run()
    rep, rec, mot = eng.report_tensors(), eng.fetch(), eng.search_motifs(["CAG"])
    assert len(rep.read) > 0
    hits = eng.search_flanks(pats)
    assert int(hits.dist[12, 0]) == 0 and int(hits.end[12, 0]) == 12
    assert _same(eng.report_tensors(), rep) and _same(eng.search_motifs(["CAG"]), mot)
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    # the search before the run: the run's records are a run's without it, and the hits are the same either side of it
    eng.upload(reads)
    first = eng.search_flanks(pats)
    eng.run()
    assert [[tuple(r) for r in rd] for rd in eng.fetch()] == [[tuple(r) for r in rd] for rd in rec]
    assert _same(first, hits) and _same(eng.search_flanks(pats), hits) and _same(eng.report_tensors(), rep)
    text = mtr_amd.format_flank_hits([f"r{i}" for i in range(len(reads))], [len(x) for x in reads], pats, hits)
    assert text.count(b"\n") == 2 * len(reads) and text.startswith(b"r0\t")
