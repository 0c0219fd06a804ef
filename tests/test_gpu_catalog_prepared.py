"""A prepared locus catalogue on the MI355X (mtr_catalog_create, mtr_genotype_catalog_prepared_device, mtr_genotype_partial_catalog_prepared_device,
Engine.build_catalog / genotype_prepared / genotype_partial_prepared, the kernels of mtr_amd/csrc/catalog_build.hip.inc).  Truth for the tables
the device builds is tests/catalog_build_ref.py, on tests/catalog_build_cases.py's sets (which tests/test_catalog_build_ref.py shows not to be
degenerate); truth for the rows is the text-taking call on the same reads and loci, column by column with torch.equal."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import catalog_build_cases as cbc
from tests import catalog_build_ref as cbr
from tests import catalog_cases as cc
from tests import flank_ref as fref
from tests import partial_catalog_cases as pcc
from tests.test_gpu_genotype import PATH_IDS, PATHS

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SETS = cbc.sets()
_REF = {}


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _texts(loci):
    return [tuple(fref.text(s) for s in locus) for locus in loci]


def _ref(name):
    if name not in _REF:
        loci, K, q = SETS[name]
        _REF[name] = cbr.build(loci, K, q)
    return _REF[name]


def _dump(eng, cat):
    """mtr_test_catalog_dump as numpy arrays (copies; the library's arrays are freed)"""
    d = mtr_amd.CCatalogDump()
    eng._check(eng.lib.mtr_test_catalog_dump(eng.h, cat.h, C.byref(d)), "mtr_test_catalog_dump")
    n, S, cap = int(d.n_loci), int(d.n_slots), int(d.table_slots)
    shapes = {"filter": (np.uint32, int(d.filter_words)), "key": (np.uint32, cap), "run": (np.int32, 2 * cap), "ent": (np.int32, int(d.entries)), "plen": (np.int32, S),
              "masks": (np.uint64, 8 * S), "units": (np.uint8, int(d.unit_bytes)), "unit_off": (np.int32, 2 * n + 1), "unit_bits": (np.uint64, 2 * n),
              "variant_bits": (np.uint64, 4 * n), "ulen": (np.int32, n)}
    free = C.CDLL(None).free
    free.argtypes = [C.c_void_p]
    out = {}
    for name, (dtype, count) in shapes.items():
        p = getattr(d, name)
        assert p, name
        out[name] = np.frombuffer(C.string_at(p, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
        free(p)
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) if hasattr(x, "dtype") else x == y for x, y in zip(a, b))


# ---- 1. the built tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
def test_the_device_builds_the_reference_s_tables(eng, name):
    loci, K, q = SETS[name]
    ref = _ref(name)
    cat = eng.build_catalog(_texts(loci), K, q)
    try:
        info = cat.info
        assert (info.n_loci, info.max_flank_dist, info.seed_len) == (len(loci), K, q) == (cat.n_loci, cat.max_flank_dist, cat.seed_len)
        assert (info.entries, info.distinct_codes, info.table_slots, info.filter_bits) == (len(ref.ent), len(ref.codes), ref.cap, ref.fbits)
        long = np.nonzero(ref.ulen > 32)[0]
        assert info.first_long_motif == (int(long[0]) if len(long) else -1) and info.device_bytes > 0
        d = _dump(eng, cat)
        assert np.array_equal(d["filter"], ref.filter)
        assert np.array_equal(d["ent"], ref.ent)
        run = d["run"].reshape(-1, 2)
        assert int((run[:, 1] != 0).sum()) == len(ref.codes)                                   # occupied slots == distinct
        first, count = cbr.probe(d["key"], run, ref.cap, ref.codes)
        assert np.array_equal(first, ref.first) and np.array_equal(count, ref.count)
        occupied = run[:, 1] != 0
        assert np.array_equal(np.sort(d["key"][occupied]), ref.codes) and not d["key"][~occupied].any() and not run[~occupied].any()
        assert np.array_equal(d["masks"].reshape(-1, 8), ref.masks) and np.array_equal(d["plen"], ref.plen)
        assert np.array_equal(d["units"], ref.units) and np.array_equal(d["unit_off"], ref.unit_off)
        assert np.array_equal(d["unit_bits"], ref.unit_bits) and np.array_equal(d["variant_bits"], ref.variant_bits) and np.array_equal(d["ulen"], ref.ulen)
    finally:
        cat.close()


def test_packed_loci_build_the_same_catalogue(eng):
    loci, K, q = SETS["edge_q16"]
    data, off = mtr_amd.pack_ids([s for locus in _texts(loci) for s in locus])
    a, b = eng.build_catalog(_texts(loci), K, q), eng.build_catalog((data, off), K, q)
    da, db = _dump(eng, a), _dump(eng, b)
    assert all(np.array_equal(da[k], db[k]) for k in da) and a.info[:8] == b.info[:8]
    a.close(), b.close()
    with pytest.raises(mtr_amd.MtrError, match="closed"):
        eng.genotype_prepared(a)
    with pytest.raises(mtr_amd.MtrError, match="seed_len"):
        eng.build_catalog((data, off), K)


# ---- 2. rows ---------------------------------------------------------------------------------------------------------------------------
def _every_arrangement(eng, monkeypatch, cat, prepared, text_taking, what):
    """one catalogue, built before any switch is set, against the text-taking call under every arrangement and both flank words"""
    rows = 0
    for word in (None, "64"):
        if word:
            monkeypatch.setenv("MTR_TEST_FLANK_WORD", word)
        for path, name in zip(PATHS, PATH_IDS):
            if path:
                monkeypatch.setenv(*path)
            got, want = prepared(cat), text_taking()
            if path:
                monkeypatch.delenv(path[0])
            assert _same(got, want), (what, name, word)
            assert got.candidates == want.candidates
            rows = got.read.numel()
        if word:
            monkeypatch.delenv("MTR_TEST_FLANK_WORD")
    return rows


@pytest.mark.parametrize("K,q", cc.KQ)
def test_the_genotype_s_rows_are_the_text_taking_call_s(eng, monkeypatch, K, q):
    loci, reads = cc.cases(K, q)
    texts = _texts(loci)
    cat = eng.build_catalog(texts, K, q)
    eng.upload(reads)
    rows = _every_arrangement(eng, monkeypatch, cat, eng.genotype_prepared, lambda: eng.genotype_catalog(texts, K, q), f"K = {K}, q = {q}")
    assert rows >= 35
    cat.close()


@pytest.mark.parametrize("K,q", pcc.KQ)
def test_the_partial_rows_are_the_text_taking_call_s(eng, monkeypatch, K, q):
    loci, reads = pcc.cases(K, q)
    texts = _texts(loci)
    cat = eng.build_catalog(texts, K, q)
    eng.upload(reads)
    rows = _every_arrangement(eng, monkeypatch, cat, eng.genotype_partial_prepared, lambda: eng.genotype_partial_catalog(texts, K, q), f"partial, K = {K}, q = {q}")
    assert rows >= 20
    for scores, tail in (((2, 1, 3), 10), ((1, 1, 1), 0)):
        assert _same(eng.genotype_partial_prepared(cat, *scores, max_tail=tail), eng.genotype_partial_catalog(texts, K, q, *scores, max_tail=tail)), (scores, tail)
    assert _same(eng.genotype_prepared(cat, 2, 1, 3), eng.genotype_catalog(texts, K, q, 2, 1, 3))
    cat.close()


# ---- 3. candidate counts ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def count_catalog(eng):
    loci, reads = cc.count_cases(257)
    cat = eng.build_catalog(_texts(loci), 2, 12)
    yield cat, _texts(loci), reads
    cat.close()


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257])
def test_counts_either_side_of_a_wavefront_and_a_workgroup(eng, count_catalog, count):
    cat, texts, reads = count_catalog
    blank = [np.zeros(50, np.uint8), np.zeros(3, np.uint8)]
    eng.upload(blank + reads[:count])
    sg = eng.genotype_prepared(cat)
    assert sg.candidates == count and sg.read.numel() == count and sg.read.tolist() == list(range(2, count + 2))
    assert _same(sg, eng.genotype_catalog(texts, 2, 12))


# ---- 4. reuse --------------------------------------------------------------------------------------------------------------------------
def test_one_catalogue_over_three_batches_with_other_calls_between(eng):
    loci, reads = pcc.cases(3, 8)
    texts = _texts(loci)
    cat = eng.build_catalog(texts, 3, 8)
    before = _dump(eng, cat)
    third = len(reads) // 3
    for k, batch in enumerate((reads[:third], reads[third:2 * third], reads[2 * third:])):
        eng.upload(batch)
        sg = eng.genotype_prepared(cat)
        eng.run()
        spg = eng.genotype_partial_prepared(cat)
        want_sg = eng.genotype_catalog(texts, 3, 8)
        again = eng.genotype_prepared(cat)
        assert _same(sg, want_sg) and _same(again, want_sg), k
        assert _same(spg, eng.genotype_partial_catalog(texts, 3, 8)), k
        assert _same(eng.genotype_partial_prepared(cat), spg), k
    after = _dump(eng, cat)
    assert all(np.array_equal(before[k], after[k]) for k in before)                        # no call wrote to the catalogue
    cat.close()


def test_two_catalogues_alternate_and_closing_one_leaves_the_other(eng):
    (l1, r1), (l2, r2) = cc.cases(1, 8), cc.cases(3, 16)
    t1, t2 = _texts(l1), _texts(l2)
    c1, c2 = eng.build_catalog(t1, 1, 8), eng.build_catalog(t2, 3, 16)
    eng.upload(r1 + r2)
    w1, w2 = eng.genotype_catalog(t1, 1, 8), eng.genotype_catalog(t2, 3, 16)
    assert w1.read.numel() >= 35 and w2.read.numel() >= 35
    for _ in range(2):
        assert _same(eng.genotype_prepared(c1), w1) and _same(eng.genotype_prepared(c2), w2)
    c1.close()
    filler = eng.build_catalog(_texts(cc.cases(0, 16)[0]), 0, 16)                              # memory of the closed one may be handed out again
    assert _same(eng.genotype_prepared(c2), w2)
    filler.close(), c2.close()


def test_a_second_engine_uses_the_first_s_catalogue_and_it_outlives_its_builder():
    loci, reads = cc.cases(1, 8)
    texts = _texts(loci)
    a, b = mtr_amd.Engine(), mtr_amd.Engine()
    try:
        cat = a.build_catalog(texts, 1, 8)                                                    # (a has no batch: none is needed)
        b.upload(reads)
        want = b.genotype_catalog(texts, 1, 8)
        assert _same(b.genotype_prepared(cat), want)
        a.upload(reads[:30])
        assert _same(a.genotype_prepared(cat), a.genotype_catalog(texts, 1, 8))
        a.close()
        assert _same(b.genotype_prepared(cat), want)
        cat.close()
        cat.close()                                                                           # closing twice is a no-op
        b.lib.mtr_catalog_destroy(None)                                                       # and so is destroying NULL
    finally:
        a.close(), b.close()


# ---- 5. scale --------------------------------------------------------------------------------------------------------------------------
def test_a_hundred_thousand_loci(eng):
    A, motifs, B, reads, carried = cc.big_catalog()
    K, q = cc.BIG_K, cc.BIG_Q
    letters = np.frombuffer(b"ACGT", np.uint8)
    flank = lambda F: [bytes(row) for row in letters[F]]      # noqa: E731
    loci = list(zip(flank(A), [bytes(letters[m]) for m in motifs], flank(B)))
    ref = cbr.build([(A[l], motifs[l], B[l]) for l in range(cc.BIG_LOCI)], K, q)
    cat = eng.build_catalog(loci, K, q)
    assert (cat.info.entries, cat.info.distinct_codes, cat.info.table_slots, cat.info.filter_bits) == (len(ref.ent), len(ref.codes), ref.cap, ref.fbits)
    d = _dump(eng, cat)
    assert np.array_equal(d["ent"], ref.ent) and np.array_equal(d["filter"], ref.filter) and np.array_equal(d["masks"].reshape(-1, 8), ref.masks)
    first, count = cbr.probe(d["key"], d["run"].reshape(-1, 2), ref.cap, ref.codes)
    assert np.array_equal(first, ref.first) and np.array_equal(count, ref.count)
    eng.upload(reads)
    sg = eng.genotype_prepared(cat)
    assert sg.candidates == len(reads) and _same(sg, eng.genotype_catalog(loci, K, q))
    cat.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def _pack(loci, off=None):
    data, o = mtr_amd.pack_ids([s for locus in loci for s in locus])
    if off is not None:
        o = np.array(off, np.int64)
    return data, o


def _text_call(eng, loci, K, q, off=None, n=None):
    data, o = _pack(loci, off)
    nr, nc = C.c_int64(-7), C.c_int64(-7)
    st = eng.lib.mtr_genotype_catalog_device(eng.h, data.ctypes.data, o.ctypes.data, len(loci) if n is None else n, K, q, 1, 1, 1, C.byref(nr), C.byref(nc))
    return mtr_amd.STATUS.get(st, st), eng.lib.mtr_last_error(eng.h).decode()


def _create(eng, loci, K, q, off=None, n=None):
    data, o = _pack(loci, off)
    h = C.c_void_p(77)
    st = eng.lib.mtr_catalog_create(eng.h, data.ctypes.data, o.ctypes.data, len(loci) if n is None else n, K, q, C.byref(h))
    if st == 0:
        eng.lib.mtr_catalog_destroy(h)
    else:
        assert not h.value
    return mtr_amd.STATUS.get(st, st), eng.lib.mtr_last_error(eng.h).decode()


OK = ("ACGTACGTACGGTCAT", "CAG", "TTGACCGATAGGCTAA")
BAD = {
    "a bad letter in a motif": dict(loci=[OK, (OK[0], "CNG", OK[2])]),
    "a bad letter in a flank": dict(loci=[OK, (OK[0], "CAG", OK[2][:7] + "x" + OK[2][8:])]),
    "a bad flank letter before a later bad motif length": dict(loci=[(OK[0][:3] + "N" + OK[0][4:], "CAG", OK[2]), (OK[0], "", OK[2])]),
    # the device finds the first bad byte, the host the first bad length; every order of the two, in the checks' order (all motifs, then the flanks)
    "a bad motif letter at a later locus against a bad flank length at an earlier one": dict(loci=[(OK[0], "CAG", ""), OK, (OK[0], "CNG", OK[2])]),
    "a bad flank letter against a later bad flank length": dict(loci=[(OK[0], "CAG", OK[2][:5] + "n" + OK[2][6:]), (OK[0], "CAG", "ACGT" * 16 + "A")]),
    "a bad flank length against a later bad flank letter": dict(loci=[("", "CAG", OK[2]), (OK[0][:2] + "N" + OK[0][3:], "CAG", OK[2])]),
    "a bad flank letter in the right flank against a bad length of the same locus' left flank": dict(loci=[OK, ("", "CAG", "NCGT" + OK[2][4:])]),
    "a bad motif length against an earlier bad motif letter": dict(loci=[(OK[0], "CAGN", OK[2]), (OK[0], "", OK[2])]),
    "a bad motif letter against an earlier bad motif length": dict(loci=[(OK[0], "ACGTC" * 100, OK[2]), (OK[0], "CxG", OK[2])]),
    "a flank of 0 bases": dict(loci=[(OK[0], "CAG", "")]),
    "a flank of 65 bases": dict(loci=[("ACGT" * 16 + "A", "CAG", OK[2])]),
    "a motif of 500 bases": dict(loci=[(OK[0], "ACGTC" * 100, OK[2])]),
    "a decreasing seq_off": dict(loci=[OK], off=[0, 16, 12, 35]),
    "a short flank for (K, q)": dict(loci=[OK, (OK[0], "CAG", OK[2][:15])]),
    "K too large for the flanks": dict(loci=[OK], K=2),
    "seed_len 7": dict(loci=[OK], q=7),
    "seed_len 17": dict(loci=[OK], q=17),
    "n_loci 0": dict(loci=[OK], n=0),
    "negative K": dict(loci=[OK], K=-1),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_create_refuses_what_the_text_taking_call_refuses_in_its_words(eng, what):
    loci, reads = cc.cases(1, 8)
    eng.upload(reads[:5])                                                  # (the text-taking call wants a batch before it looks at its loci)
    kw = {"K": 1, "q": 8, **BAD[what]}
    want = _text_call(eng, **kw)
    assert want[0] == "MTR_ERR_BAD_ARG", (what, want)
    assert _create(eng, **kw) == want, what


def _prepared_raw(eng, cat, partial=False, scores=(1, 1, 1), max_tail=10):
    nr, nc = C.c_int64(-7), C.c_int64(-7)
    if partial:
        st = eng.lib.mtr_genotype_partial_catalog_prepared_device(eng.h, cat.h, *scores, max_tail, C.byref(nr), C.byref(nc))
    else:
        st = eng.lib.mtr_genotype_catalog_prepared_device(eng.h, cat.h, *scores, C.byref(nr), C.byref(nc))
    return mtr_amd.STATUS.get(st, st), int(nr.value), int(nc.value), eng.lib.mtr_last_error(eng.h).decode()


def _kept(eng, partial):
    """whether the context still hands out rows of that kind: the copy's answer to a destination without room"""
    if partial:
        st = eng.lib.mtr_genotype_partial_catalog_copy_device(eng.h, C.byref(mtr_amd.CPartialCatalogDst(None, None, mtr_amd.CPartialDst(*[None] * 7, -1))))
    else:
        st = eng.lib.mtr_genotype_catalog_copy_device(eng.h, C.byref(mtr_amd.CCatalogDst(None, None, mtr_amd.CGenotypesDst(*[None] * 7, -1))))
    return mtr_amd.STATUS[st] != "MTR_ERR_BAD_ARG" or "comes first" not in eng.lib.mtr_last_error(eng.h).decode()


def test_the_prepared_calls_refuse_in_the_text_taking_calls_words():
    loci, reads = pcc.cases(3, 8)
    texts = _texts(loci)
    long_loci = texts[:2] + [(texts[2][0], "ACGTT" * 6 + "ACG", texts[2][2])]                      # a motif of 33 bases at locus 2
    e = mtr_amd.Engine()
    try:
        cat, cat33 = e.build_catalog(texts, 3, 8), e.build_catalog(long_loci, 3, 8)
        assert cat33.info.first_long_motif == 2 and cat.info.first_long_motif == -1
        for partial in (False, True):
            st, R, Cn, msg = _prepared_raw(e, cat, partial)
            assert (st, R, Cn, msg) == ("MTR_ERR_BAD_ARG", 0, 0, "no batch uploaded")
        e.upload(reads)
        data, o = _pack(texts)
        for partial in (False, True):
            for kw, word in ((dict(scores=(0, 1, 1)), "gain = 0 outside 1..5"), (dict(scores=(1, 4, 1)), "mismatch = 4 outside 1..3"), (dict(scores=(1, 1, 0)), "indel = 0 outside 1..3")):
                assert _prepared_raw(e, cat, partial)[0] == "MTR_OK" and _kept(e, partial)
                st, R, Cn, msg = _prepared_raw(e, cat, partial, **kw)
                assert (st, R, Cn, msg) == ("MTR_ERR_BAD_ARG", 0, 0, word), (partial, kw, msg)
                assert not _kept(e, partial)                                               # as the text-taking call: a failed call keeps nothing
        # the text-taking partial call's words for max_tail < 0 and for the motif of 33 bases
        def text_partial(tx, max_tail):
            d, off = _pack(tx)
            nr, nc = C.c_int64(), C.c_int64()
            st = e.lib.mtr_genotype_partial_catalog_device(e.h, d.ctypes.data, off.ctypes.data, len(tx), 3, 8, 1, 1, 1, max_tail, C.byref(nr), C.byref(nc))
            return mtr_amd.STATUS.get(st, st), e.lib.mtr_last_error(e.h).decode()

        assert _prepared_raw(e, cat, True, max_tail=-1)[0::3] == text_partial(texts, -1) and "max_tail = -1" in e.lib.mtr_last_error(e.h).decode()
        assert _prepared_raw(e, cat33, True)[0::3] == text_partial(long_loci, 10) and "locus 2" in e.lib.mtr_last_error(e.h).decode()
        assert _prepared_raw(e, cat33, True, max_tail=-1)[0::3] == text_partial(long_loci, -1)    # the motif comes before max_tail
        assert _same(e.genotype_prepared(cat33), e.genotype_catalog(long_loci, 3, 8))             # the genotype takes the long motif
        assert _same(e.genotype_partial_prepared(cat), e.genotype_partial_catalog(texts, 3, 8))   # and the context is usable after the refusals
        cat.close(), cat33.close()
    finally:
        e.close()


def test_dp_too_large_comes_where_the_text_taking_call_gives_it(monkeypatch):
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(65 * 300 + 64))
    e = mtr_amd.Engine()
    try:
        rng = np.random.RandomState(8)
        e.upload([rng.randint(0, 4, size=L).astype(np.uint8) for L in (100, 299, 300, 50)])
        t = lambda n: fref.text(rng.randint(0, 4, size=n))      # noqa: E731
        loci = [(t(20), "CAG", t(20)), (t(20), t(63), t(20)), (t(20), t(64), t(20))]
        for sub in (loci, loci[:1], loci[:2], loci[1:], loci[2:]):
            cat = e.build_catalog(sub, 1, 8)                                                  # the build knows no read: it takes them all
            want = _text_call(e, sub, 1, 8)
            got = _prepared_raw(e, cat)
            assert (got[0], got[3] if got[0] != "MTR_OK" else want[1]) == want, sub
            assert _prepared_raw(e, cat, scores=(0, 1, 1))[0] == ("MTR_ERR_DP_TOO_LARGE" if want[0] == "MTR_ERR_DP_TOO_LARGE" else "MTR_ERR_BAD_ARG")   # the size before the scores
            # the partial call stores no cell: no such refusal - it answers, or refuses the motifs of 63 and 64 bases as its own
            assert _prepared_raw(e, cat, True)[0] == ("MTR_OK" if all(len(m) <= 32 for _, m, _ in sub) else "MTR_ERR_BAD_ARG")
            cat.close()
        assert _text_call(e, loci, 1, 8)[0] == "MTR_ERR_DP_TOO_LARGE"
    finally:
        e.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                                                         # the device's limit back to the built-in one


def test_a_context_on_another_device_is_refused():
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    loci, reads = cc.cases(1, 8)
    a, b = mtr_amd.Engine(device=0), mtr_amd.Engine(device=1)
    try:
        cat = a.build_catalog(_texts(loci), 1, 8)
        b.upload(reads)
        for partial in (False, True):
            st, _, _, msg = _prepared_raw(b, cat, partial)
            assert st == "MTR_ERR_BAD_ARG" and "device" in msg
        cat.close()
    finally:
        a.close(), b.close()


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
def test_two_batches_joined_give_the_text_taking_call_s_alleles(eng):
    loci, reads = cc.cases(1, 8)
    texts = _texts(loci)
    cat = eng.build_catalog(texts, 1, 8)
    half = len(reads) // 2

    def joined(call):
        parts, first = [], 0
        for batch in (reads[:half], reads[half:]):
            eng.upload(batch)
            sg = call()
            parts.append(sg._replace(read=sg.read + first))
            first += len(batch)
        return mtr_amd.SparseGenotypes(first, len(loci), *[torch.cat([p[k] for p in parts]) for k in range(2, 11)], sum(p.candidates for p in parts))

    got, want = joined(lambda: eng.genotype_prepared(cat)), joined(lambda: eng.genotype_catalog(texts, 1, 8))
    assert _same(got, want) and got.read.numel() >= 35
    calls, calls_want = eng.call_alleles(got, min_support=1), eng.call_alleles(want, min_support=1)
    assert all(torch.equal(a, b) for a, b in zip(calls, calls_want))
    assert all(torch.equal(a, b) for a, b in zip(calls, eng.call_alleles(eng_all(eng, reads, texts), min_support=1)))
    cat.close()


def eng_all(eng, reads, texts):
    """the same rows from one batch of all the reads"""
    eng.upload(reads)
    return eng.genotype_catalog(texts, 1, 8)
