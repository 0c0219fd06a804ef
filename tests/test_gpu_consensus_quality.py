"""The qualities of the resident batch, their windows and the quality-weighted allele consensus on the MI355X (mtr_keep_qualities,
mtr_attach_qualities_device, mtr_extract_window_qualities_device, mtr_allele_consensus_quality_device; the kernels of mtr_amd/csrc/quality.hip.inc
and consensus_quality.hip.inc).

Truth is tests/consensus_quality_ref.py, the definition of include/mtr_hip.h in plain Python; tests/test_consensus_quality_ref.py holds it to
answers worked out on paper and to its two properties.  Everything is exact equality: every column, every dtype, every shape."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import mtr_amd
from tests import consensus_cases as cc
from tests import consensus_quality_cases as qc
from tests import consensus_quality_ref as qref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CAPS = (1, 10, 40)
CASES = [(name, cap) for name in sorted(cc.all_cases()) for cap in CAPS if name != "limit"] + [("limit", 40)]      # the window limit runs once


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", eng.device))


def _inputs(eng, case, qual):
    sg = SimpleNamespace(n_loci=case["n_loci"], read=_dev(eng, case["read"]), locus=_dev(eng, case["locus"]))
    win = mtr_amd.GenotypeWindows(_dev(eng, case["win_off"]), _dev(eng, case["win_bases"]))
    calls = SimpleNamespace(support_off=_dev(eng, case["support_off"]), read=_dev(eng, case["sup_read"]), allele=_dev(eng, case["allele"]), zygosity=_dev(eng, case["zygosity"]))
    return sg, win, _dev(eng, qual), calls


def _assert_cons(got, want, what=""):
    for name, g, w in zip(mtr_amd.AlleleConsensus._fields, (t.cpu().numpy() for t in got), want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError((what, name, at.tolist(), g[tuple(at)].tolist(), w[tuple(at)].tolist()))


@pytest.mark.parametrize("name,cap", CASES)
def test_every_column_equals_the_reference(eng, name, cap):
    case, qual, want = qref.expected(name, cap)
    assert int(qual.max()) <= 60
    got = eng.allele_consensus_quality(*_inputs(eng, case, qual), band_extra=case["band_extra"], qual_cap=cap)
    _assert_cons(got, want, (name, cap))
    again = eng.allele_consensus_quality(*_inputs(eng, case, qual), band_extra=case["band_extra"], qual_cap=cap)
    assert all(torch.equal(x, y) for x, y in zip(got, again)), name


@pytest.mark.parametrize("name", sorted(cc.all_cases()))
def test_cap_one_is_the_unweighted_call_in_all_eight_columns(eng, name):
    case = cc.all_cases()[name]
    qual = qref.seeded_qualities(case, 99)
    sg, win, q, calls = _inputs(eng, case, qual)
    plain = eng.allele_consensus(sg, win, calls, band_extra=case["band_extra"])
    got = eng.allele_consensus_quality(sg, win, q, calls, band_extra=case["band_extra"], qual_cap=1)
    assert len(got) == 8 and all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(got, plain)), name


@pytest.mark.parametrize("name", sorted(qc.hand_cases()))
def test_the_hand_cases_give_their_paper_answers(eng, name):
    members, cap, (bases, votes), plain = qc.hand_cases()[name]
    case, qual = qc.hand_case_columns(members)
    sg, win, q, calls = _inputs(eng, case, qual)
    got = eng.allele_consensus_quality(sg, win, q, calls, band_extra=16, qual_cap=cap)
    assert got.bases.cpu().tolist() == bases and got.votes.cpu().tolist() == votes and got.off.cpu().tolist() == [0, len(bases), len(bases)]
    assert eng.allele_consensus(sg, win, calls, band_extra=16).bases.cpu().tolist() == plain


# ---- the quality windows ------------------------------------------------------------------------------------------------------------------------
def _quality_reads():
    """reads of 1 .. 200 bases whose quality bytes are 32, 33, 126 and 127 at the ends and among seeded ones"""
    rng = np.random.default_rng(31)
    reads = []
    for n in (1, 63, 64, 65, 200, 130, 7):
        q = rng.integers(33, 127, size=n).astype(np.uint8)
        q[rng.integers(0, n, size=max(n // 4, 1))] = rng.choice(np.array([32, 33, 126, 127], np.uint8), size=max(n // 4, 1))
        q[0], q[-1] = (32, 127) if len(reads) % 2 else (126, 33)
        reads.append((cc.seq(rng, n), q))
    return reads


def _fastq_of(reads_ascii_q):
    out = bytearray()
    for k, (r, q) in enumerate(reads_ascii_q):
        out += f"@q{k}\n".encode() + bytes(cc.LETTERS[c].encode()[0] for c in r) + b"\n+\n" + bytes(q.tolist()) + b"\n"
    return bytes(out)


def _phred(ascii_bytes):
    return np.clip(np.asarray(ascii_bytes, np.int32) - 33, 0, 93).astype(np.uint8)


def _quality_rows():
    rows = []
    for n in (0, 1, 63, 64, 65):                         # every length at starts of every residue of a dword, in both orientations
        for lo in (0, 1, 2, 3, 5):
            for rd, size in ((4, 200), (5, 130)):
                if lo + n <= size:
                    rows += [(rd, lo, lo + n, 0), (rd, size - n - lo, size - lo, 1)]
    rows += [(0, 0, 1, 1), (0, 1, 1, 0), (1, 0, 63, 1), (2, 0, 64, 1), (3, 0, 65, 0), (3, 1, 65, 1), (6, 2, 2, 1), (4, 0, 200, 1)]
    return sorted(set(rows))


def _rows_namespace(eng, rows):
    col = lambda k, dt: _dev(eng, np.array([r[k] for r in rows], dt).reshape(len(rows)))      # noqa: E731
    return SimpleNamespace(read=col(0, np.int32), orientation=col(3, np.uint8), window=_dev(eng, np.array([[r[1], r[2]] for r in rows], np.int32).reshape(len(rows), 2)))


def _dev_bytes(eng, data):
    return _dev(eng, np.frombuffer(data, np.uint8).copy())


def test_the_quality_windows_equal_slicing_on_the_host(eng):
    reads, rows = _quality_reads(), _quality_rows()
    f = eng.upload_fastq_device(_dev_bytes(eng, _fastq_of(reads)), keep_quality=True)
    assert f.end == "eof" and len(f.lens) == len(reads) and eng.qualities_resident() == sum(len(r) for r, _ in reads)
    ns = _rows_namespace(eng, rows)
    win, got = eng.genotype_windows(ns), eng.genotype_window_qualities(ns)
    want = [_phred(reads[r][1])[lo:hi][::-1] if o else _phred(reads[r][1])[lo:hi] for r, lo, hi, o in rows]
    assert {len(w) for w in want} >= {0, 1, 63, 64, 65} and {0, 93} <= set(np.concatenate(want).tolist())
    assert got.dtype == torch.uint8 and got.numel() == win.bases.numel() == int(win.off[-1])
    assert got.cpu().numpy().tolist() == np.concatenate(want).tolist()
    assert win.bases.cpu().numpy().tolist() == np.concatenate([cc.oriented_window(reads[r][0], lo, hi, o) for r, lo, hi, o in rows]).tolist()
    assert eng.genotype_window_qualities(_rows_namespace(eng, [])).numel() == 0


def test_attached_qualities_give_the_windows_of_the_fastq_route(eng):
    reads, rows = _quality_reads(), _quality_rows()
    eng.upload_fastq_device(_dev_bytes(eng, _fastq_of(reads)), keep_quality=True)
    ns = _rows_namespace(eng, rows)
    by_fastq = eng.genotype_window_qualities(ns)
    lens = np.array([len(r) for r, _ in reads], np.int32)
    text_off = np.zeros(len(reads), np.int64)
    text_off[1:] = np.cumsum(lens[:-1])
    eng.upload_device(_dev(eng, np.concatenate([r for r, _ in reads])), text_off, lens, codes=True)
    assert eng.qualities_resident() == 0
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: no qualities resident"):
        eng.genotype_window_qualities(ns)
    # the caller's values with a gap of three bytes in front of every read, raw values above 93 among them (126 - 33 = 93 is stored for 127 - 33 = 94)
    phred = [np.clip(q.astype(np.int32) - 33, 0, 255).astype(np.uint8) for _, q in reads]
    offs = np.cumsum([3] + [len(p) + 3 for p in phred[:-1]]).astype(np.int64)
    blob = np.full(int(offs[-1]) + len(phred[-1]), 200, np.uint8)
    for o, p in zip(offs, phred):
        blob[o:o + len(p)] = p
    d_blob = _dev(eng, blob)
    eng.attach_qualities(d_blob, offs)
    assert eng.qualities_resident() == int(lens.sum())
    assert torch.equal(eng.genotype_window_qualities(ns), by_fastq)
    for bad, word in ((np.where(np.arange(len(offs)) == 2, len(blob) - 10, offs), "read 2: values"), (np.where(np.arange(len(offs)) == 1, -1, offs), "read 1: values")):
        with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: {word}"):
            eng.attach_qualities(d_blob, bad)
    assert torch.equal(eng.genotype_window_qualities(ns), by_fastq)                 # a refused attach leaves the qualities as they were
    assert mtr_amd.STATUS[eng.lib.mtr_attach_qualities_device(eng.h, blob.ctypes.data, len(blob), offs.ctypes.data, None)] == "MTR_ERR_BAD_ARG"
    assert "d_qual is not device memory" in eng.lib.mtr_last_error(eng.h).decode()
    assert mtr_amd.STATUS[eng.lib.mtr_attach_qualities_device(eng.h, None, len(blob), offs.ctypes.data, None)] == "MTR_ERR_BAD_ARG"
    assert mtr_amd.STATUS[eng.lib.mtr_attach_qualities_device(eng.h, d_blob.data_ptr(), 1 << 40, offs.ctypes.data, None)] == "MTR_ERR_BAD_ARG"
    assert "runs past the end" in eng.lib.mtr_last_error(eng.h).decode()
    fresh = mtr_amd.Engine()
    assert mtr_amd.STATUS[fresh.lib.mtr_attach_qualities_device(fresh.h, d_blob.data_ptr(), len(blob), offs.ctypes.data, None)] == "MTR_ERR_BAD_ARG"
    assert "no batch uploaded" in fresh.lib.mtr_last_error(fresh.h).decode()
    fresh.close()


def test_the_quality_windows_protocol_and_what_drops_the_qualities(eng):
    reads, rows = _quality_reads(), _quality_rows()
    buf = _dev_bytes(eng, _fastq_of(reads))
    ns = _rows_namespace(eng, rows)
    R, T = len(rows), sum(r[2] - r[1] for r in rows)
    dst = torch.full((T,), 77, dtype=torch.uint8, device=torch.device("cuda", eng.device))
    nb = C.c_int64()
    call = lambda d, cap: eng.lib.mtr_extract_window_qualities_device(eng.h, ns.read.data_ptr(), ns.orientation.data_ptr(), ns.window.data_ptr(), R, None, d, cap, C.byref(nb))      # noqa: E731
    torch.cuda.synchronize()
    fresh = mtr_amd.Engine()
    with pytest.raises(mtr_amd.MtrError, match="no batch uploaded"):
        fresh.genotype_window_qualities(_rows_namespace(fresh, rows))
    fresh.close()
    eng.upload_fastq_device(buf)                                                      # the option is off: a batch, no qualities
    assert eng.qualities_resident() == 0 and mtr_amd.STATUS[call(dst.data_ptr(), T)] == "MTR_ERR_BAD_ARG" and b"no qualities resident" in eng.lib.mtr_last_error(eng.h)
    eng.upload_fastq_device(buf, keep_quality=True)
    assert eng.qualities_resident() > 0 and call(None, 0) == 0 and nb.value == T
    assert mtr_amd.STATUS[call(dst.data_ptr(), T - 1)] == "MTR_ERR_OVERFLOW" and nb.value == T
    for bad in ((8, 0, 1, 0), (4, 5, 201, 0), (4, 9, 8, 1)):                         # the windows' own refusals, in their words
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: row 2:"):
            eng.genotype_window_qualities(_rows_namespace(eng, rows[:2] + [bad] + rows[2:]))
    assert mtr_amd.STATUS[eng.lib.mtr_extract_window_qualities_device(eng.h, ns.read.data_ptr(), None, ns.window.data_ptr(), R, None, dst.data_ptr(), T, C.byref(nb))] == "MTR_ERR_BAD_ARG"
    assert (dst == 77).all()
    assert call(dst.data_ptr(), T) == 0 and torch.equal(dst, eng.genotype_window_qualities(ns))
    eng.upload_fastq_device(buf)                                                      # an upload with the option off after one with it leaves none
    assert eng.qualities_resident() == 0
    with pytest.raises(mtr_amd.MtrError, match="no qualities resident"):
        eng.genotype_window_qualities(ns)
    eng.upload_fastq_device(buf, keep_quality=True)
    fasta = b"".join(f">r{k}\n".encode() + bytes(cc.LETTERS[c].encode()[0] for c in r) + b"\n" for k, (r, _) in enumerate(reads))
    assert len(eng.upload_fasta_device(_dev_bytes(eng, fasta)).lens) == len(reads)   # a FASTA upload leaves none
    assert eng.qualities_resident() == 0
    with pytest.raises(mtr_amd.MtrError, match="no qualities resident"):
        eng.genotype_window_qualities(ns)
    assert eng.genotype_windows(ns).bases.numel() == T                                # and the next call succeeds


# ---- from FASTQ bytes to alleles ------------------------------------------------------------------------------------------------------------------
def _genotyped(eng, loci):
    sg = eng.genotype_loci(loci, 1).to_sparse()
    return sg, eng.genotype_windows(sg), eng.genotype_window_qualities(sg)


def _consensus_of_parts(eng, parts):
    sg, win = mtr_amd.join_sparse_genotypes([p[0] for p in parts]), mtr_amd.join_windows([p[1] for p in parts])
    qual = mtr_amd.join_window_qualities([p[2] for p in parts], win)
    calls = eng.call_alleles(sg, "bases")
    return sg, win, qual, calls, eng.allele_consensus_quality(sg, win, qual, calls, band_extra=qc.FQ_EXTRA, qual_cap=qc.FQ_CAP)


def test_from_fastq_bytes_to_the_true_alleles_in_one_batch_and_in_two(eng):
    """seed qc.FQ_SEED = 11: five reads an allele at 6 % errors, where the unweighted consensus misses a true allele and the weighted one is both"""
    reads, loci, truth = qc.fq_reads(), cc.truth_loci(), cc.truth_alleles()
    buf = _dev_bytes(eng, qc.fastq_bytes(reads))
    f = eng.upload_fastq_device(buf, keep_quality=True)
    assert f.end == "eof" and len(f.lens) == 2 * qc.FQ_READS
    sg, win, qual, calls, cons = _consensus_of_parts(eng, [_genotyped(eng, loci)])
    n = 2 * qc.FQ_READS
    assert sg.read.cpu().tolist() == list(range(n)) and sg.locus.cpu().tolist() == [0] * n and sg.orientation.cpu().tolist() == [k % 2 for k in range(n)]
    case, case_qual = qc.fq_case()
    assert win.off.cpu().tolist() == case["win_off"].tolist() and win.bases.cpu().numpy().tolist() == case["win_bases"].tolist()
    assert qual.cpu().numpy().tolist() == case_qual.tolist()
    assert calls.zygosity.cpu().tolist() == [2, 0] and calls.read.cpu().tolist() == case["sup_read"].tolist() and calls.allele.cpu().tolist() == case["allele"].tolist()
    off = cons.off.cpu().tolist()
    for a in (0, 1):
        assert cons.bases[off[a]:off[a + 1]].cpu().tolist() == truth[a].tolist(), a
    _assert_cons(cons, qref.consensus(case, case_qual, qc.FQ_EXTRA, qc.FQ_CAP), "one batch")
    plain = eng.allele_consensus(sg, win, calls, band_extra=qc.FQ_EXTRA)
    poff = plain.off.cpu().tolist()
    assert [plain.bases[poff[a]:poff[a + 1]].cpu().tolist() for a in (0, 1)] != [t.tolist() for t in truth]      # one vote a base misses an allele here
    text = mtr_amd.format_allele_consensus(loci, cons).decode().splitlines()
    assert len(text) == 2 and text[0].split("\t")[6] == "".join(cc.LETTERS[c] for c in truth[0])
    parts = []
    for item in eng.walk_fastq_device(buf, 2500, keep_quality=True):
        if len(item.lens):
            parts.append(_genotyped(eng, loci))
    assert len(parts) >= 2
    two = _consensus_of_parts(eng, parts)
    assert torch.equal(two[2], qual) and all(torch.equal(x, y) for x, y in zip(two[1], win)) and all(torch.equal(x, y) for x, y in zip(two[4], cons))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_the_refusals_write_nothing_and_the_next_call_succeeds(eng):
    case, qual, want = qref.expected("members", 40)
    sg, win, q, calls = _inputs(eng, case, qual)
    swapped = case["read"].copy()
    swapped[[4, 5]] = swapped[[5, 4]]
    locus_swapped = case["locus"].copy()
    locus_swapped[[4, 5]] = locus_swapped[[5, 4]]
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: row 5 is out of order"):
        eng.allele_consensus_quality(SimpleNamespace(n_loci=sg.n_loci, read=_dev(eng, swapped), locus=_dev(eng, locus_swapped)), win, q, calls, band_extra=8)
    lost = case["sup_read"].copy()
    lost[7] = int(case["read"].max()) + 1
    with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: support entry 7 \(read \d+\) has no row"):
        eng.allele_consensus_quality(sg, win, q, SimpleNamespace(support_off=calls.support_off, read=_dev(eng, lost), allele=calls.allele, zygosity=calls.zygosity), band_extra=8)
    for extra in (-1, mtr_amd.CONS_MAX_EXTRA + 1):
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: band_extra"):
            eng.allele_consensus_quality(sg, win, q, calls, band_extra=extra)
    for cap in (0, mtr_amd.CONSQ_MAX_CAP + 1):
        with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: qual_cap = {cap} outside 1..93"):
            eng.allele_consensus_quality(sg, win, q, calls, band_extra=8, qual_cap=cap)
    G, T = 2 * case["n_loci"], len(want[1])
    dev = torch.device("cuda", eng.device)
    shapes = ((G + 1, torch.int64), (T, torch.uint8), (T, torch.int32)) + ((G, torch.int32),) * 5
    cols = [torch.full((n,), 77, dtype=t, device=dev) for n, t in shapes]
    make_src = lambda n_support: mtr_amd.CConsensusSrc(sg.read.data_ptr(), sg.locus.data_ptr(), win.off.data_ptr(), win.bases.data_ptr(), calls.support_off.data_ptr(),      # noqa: E731
                                                       calls.read.data_ptr(), calls.allele.data_ptr(), calls.zygosity.data_ptr(), sg.read.numel(), win.bases.numel(), n_support,
                                                       case["n_loci"])
    src = make_src(calls.read.numel())
    nb = C.c_int64()
    call = lambda dst, extra=8, cap=40, qp=q.data_ptr(), s=src: eng.lib.mtr_allele_consensus_quality_device(eng.h, C.byref(s), qp, extra, cap, None, dst, C.byref(nb))      # noqa: E731
    ptrs = [c.data_ptr() for c in cols]
    full = C.byref(mtr_amd.CConsensusDst(*ptrs, G, T))
    torch.cuda.synchronize()
    assert call(None) == 0 and nb.value == T
    for cap_alleles, cap_bases in ((G - 1, T), (G, T - 1)):
        assert mtr_amd.STATUS[call(C.byref(mtr_amd.CConsensusDst(*ptrs, cap_alleles, cap_bases)))] == "MTR_ERR_OVERFLOW" and nb.value == T
    assert mtr_amd.STATUS[call(C.byref(mtr_amd.CConsensusDst(*ptrs[:2], None, *ptrs[3:], G, T)))] == "MTR_ERR_BAD_ARG"
    assert mtr_amd.STATUS[call(full, 65)] == "MTR_ERR_BAD_ARG"
    assert mtr_amd.STATUS[call(full, 8, 0)] == "MTR_ERR_BAD_ARG" and mtr_amd.STATUS[call(full, 8, 94)] == "MTR_ERR_BAD_ARG"
    # the sums are int32: n_support * qual_cap must stay below 2^31 (refused before a column is looked at)
    many = -(-(1 << 31) // 40)
    assert mtr_amd.STATUS[call(full, 8, 40, s=make_src(many))] == "MTR_ERR_BAD_ARG" and b"reaches 2^31" in eng.lib.mtr_last_error(eng.h)
    assert mtr_amd.STATUS[call(full, qp=None)] == "MTR_ERR_BAD_ARG" and b"an input column is NULL" in eng.lib.mtr_last_error(eng.h)
    assert mtr_amd.STATUS[call(full, qp=qual.ctypes.data)] == "MTR_ERR_BAD_ARG" and b"win_qual is not device memory" in eng.lib.mtr_last_error(eng.h)
    assert all((c == 77).all() for c in cols)
    assert call(full) == 0
    _assert_cons(cols, want, "after the refusals")
