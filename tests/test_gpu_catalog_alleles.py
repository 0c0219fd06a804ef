"""Allele calls from sparse rows on the MI355X (mtr_call_alleles_rows_device, Engine.call_alleles on a SparseGenotypes).  Truth is
Engine.call_alleles on the dense rows: every column must be torch.equal.  The inputs are tests/allele_call_cases.py's turned into row lists - the
spanning rows in a shuffled order, with a few rows that span nothing among them - and the reads of its end-to-end case through
genotype_catalog, as one batch and as two batches joined."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import allele_call_cases as cases
from tests import flank_ref as fref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _dense(rows, eng):
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return mtr_amd.Genotypes(t(rows.spanning), None, None, t(rows.window), t(rows.fields), None, t(rows.ratio))


def _sparse(rows, eng, seed=5, extra=7):
    """the spanning rows of a dense input and `extra` rows that span nothing, in a shuffled order"""
    rng = np.random.RandomState(seed)
    n, m = rows.spanning.shape
    at = np.argwhere(rows.spanning == 1)
    idle = np.argwhere(rows.spanning != 1)
    at = np.concatenate([at, idle[rng.choice(len(idle), size=min(extra, len(idle)), replace=False)]]) if len(idle) else at
    at = at[rng.permutation(len(at))]
    r, l = at[:, 0], at[:, 1]
    dev = torch.device("cuda", eng.device)
    t = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(dev)      # noqa: E731
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)      # noqa: E731
    return mtr_amd.SparseGenotypes(n, m, t(r, np.int32), t(l, np.int32), t(rows.spanning[r, l], np.uint8), torch.zeros(len(at), dtype=torch.uint8, device=dev),
                                   zeros(len(at), 2), t(rows.window[r, l], np.int32), t(rows.fields[r, l], np.int32), zeros(len(at)), t(rows.ratio[r, l], np.float32), 0)


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["hand", "lane_63", "lane_64", "many_loci", "spread_4097", "tile_edges", "empty_windows", "smallest", "nothing"])
def test_the_calls_from_sparse_rows_are_the_dense_calls(eng, name):
    rows = {"hand": cases.from_lists, "lane_63": lambda: cases.lane_edges(63), "lane_64": lambda: cases.lane_edges(64), "many_loci": cases.many_loci,
            "spread_4097": lambda: cases.spread_edges(cases.SPREAD_LOCI + 1), "tile_edges": cases.tile_edges, "empty_windows": cases.empty_windows,
            "smallest": lambda: cases.smallest(True), "nothing": lambda: cases.smallest(False)}[name]()
    gt, sg = _dense(rows, eng), _sparse(rows, eng, extra=0 if name == "nothing" else 7)
    assert sg.read.numel() == (0 if name == "nothing" else int(rows.spanning.sum()) + min(7, int((rows.spanning != 1).sum())))
    for measure in ("copies", "bases"):
        for rule in cases.SWEEP[:2]:
            ratio = 1.0 if name == "empty_windows" else cases.MIN_RATIO
            want = eng.call_alleles(gt, measure, ratio, *rule)
            assert _same(eng.call_alleles(sg, measure, ratio, *rule), want), (name, measure, rule)
    assert name in ("nothing",) or int(want.support_off[-1]) >= 1


def _texts(loci):
    return [tuple(fref.text(s) for s in locus) for locus in loci]


def test_reads_to_catalogue_to_alleles_in_one_batch_and_in_two(eng):
    reads, loci = cases.e2e()
    texts = _texts(loci)
    eng.upload(reads)
    dense, sg = eng.genotype_loci(texts, 1), eng.genotype_catalog(texts, 1, 8)
    assert sg.read.numel() == int(dense.spanning.sum()) >= 20
    want = {m: eng.call_alleles(dense, m, cases.E2E_MIN_RATIO, *cases.E2E_RULE) for m in ("copies", "bases")}
    assert int(want["copies"].support_off[-1]) >= 15 and int(want["copies"].zygosity.max()) >= 1
    for m in want:
        assert _same(eng.call_alleles(sg, m, cases.E2E_MIN_RATIO, *cases.E2E_RULE), want[m]), m
    parts, base = [], 0
    for batch in (reads[:11], reads[11:]):
        eng.upload(batch)
        part = eng.genotype_catalog(texts, 1, 8)
        parts.append(part._replace(read=part.read + base))
        base += len(batch)
    joined = mtr_amd.SparseGenotypes(base, len(loci), *[torch.cat(cols) for cols in zip(*[p[2:11] for p in parts])], sum(p.candidates for p in parts))
    assert _same(joined[2:11], sg[2:11]) and joined.candidates == sg.candidates
    for m in want:
        assert _same(eng.call_alleles(joined, m, cases.E2E_MIN_RATIO, *cases.E2E_RULE), want[m]), m


def test_a_duplicate_pair_and_a_locus_out_of_range_are_refused_and_nothing_is_written(eng):
    rows = cases.from_lists()
    sg = _sparse(rows, eng)
    good = eng.call_alleles(sg, "copies", cases.MIN_RATIO, 1, 0, 1)
    m, S, dev = sg.n_loci, int(good.support_off[-1]), torch.device("cuda", eng.device)
    prm = mtr_amd.CAlleleParams(mtr_amd.ALLELE_COPIES, cases.MIN_RATIO, 1, 0, 1)

    def raw(read, locus, dst=True, n_loci=m):
        R = read.numel()
        cols = [torch.full(shape, 77, dtype=t, device=dev) for shape, t in (((m + 1,), torch.int64), ((S,), torch.int32), ((S,), torch.int32), ((S,), torch.uint8),
                                                                              ((m,), torch.uint8), ((m, 2), torch.int32), ((m, 2), torch.int32), ((m, 2), torch.int64))]
        torch.cuda.synchronize()
        r = mtr_amd.CGenotypesDst(sg.spanning.data_ptr(), None, None, sg.window.data_ptr(), sg.fields.data_ptr(), None, sg.ratio.data_ptr(), R)
        d = mtr_amd.CAlleleCallsDst(*[c.data_ptr() for c in cols], m, S)
        ns = C.c_int64(-7)
        st = eng.lib.mtr_call_alleles_rows_device(eng.h, C.byref(r), read.data_ptr(), locus.data_ptr(), R, n_loci, C.byref(prm), None, C.byref(d) if dst else None, C.byref(ns))
        torch.cuda.synchronize()
        return mtr_amd.STATUS.get(st, st), eng.lib.mtr_last_error(eng.h).decode(), cols, int(ns.value)

    st, _, cols, ns = raw(sg.read, sg.locus)
    assert st == "MTR_OK" and ns == S and _same(cols, good)
    # a supporting row's (locus, read) a second time, far from the first
    first = int(torch.nonzero(sg.spanning == 1)[0])
    read, locus = sg.read.clone(), sg.locus.clone()
    other = (first + sg.read.numel() // 2) % sg.read.numel()
    read[other], locus[other] = read[first], locus[first]
    for dst in (True, False):
        st, msg, cols, ns = raw(read, locus, dst)
        assert st == "MTR_ERR_BAD_ARG" and f"(locus {int(locus[first])}, read {int(read[first])})" in msg and "more than one row" in msg and ns == 0, (st, msg)
        assert all(bool((c == 77).all()) for c in cols)
    for bad in (m, -1, 2 ** 31 - 1):
        locus = sg.locus.clone()
        locus[3] = bad
        st, msg, cols, ns = raw(sg.read, locus)
        assert st == "MTR_ERR_BAD_ARG" and msg.startswith("row 3:") and f"locus {bad}" in msg and ns == 0, (st, msg)
        assert all(bool((c == 77).all()) for c in cols)
    read = sg.read.clone()
    read[5] = -2
    st, msg, cols, _ = raw(read, sg.locus)
    assert st == "MTR_ERR_BAD_ARG" and msg.startswith("row 5:") and all(bool((c == 77).all()) for c in cols)
    st, msg, _, _ = raw(sg.read, sg.locus, n_loci=0)
    assert st == "MTR_ERR_BAD_ARG" and "n_loci" in msg
    with pytest.raises(mtr_amd.MtrError, match="more than one row"):
        eng.call_alleles(sg._replace(read=torch.cat([sg.read[:1], sg.read[:-1]]), locus=torch.cat([sg.locus[:1], sg.locus[:-1]])), "copies", cases.MIN_RATIO, 1, 0, 1)
    with pytest.raises(mtr_amd.MtrError):
        eng.call_alleles(sg._replace(read=sg.read.long()), "copies")
    assert _same(eng.call_alleles(sg, "copies", cases.MIN_RATIO, 1, 0, 1), good)
