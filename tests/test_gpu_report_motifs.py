"""The motif catalogue on the MI355X (mtr_report_motifs_device, Engine.report_motif_tensors, the kernels of mtr_amd/csrc/report_motif.hip.inc).

The reference has no such output: truth is the brute force of tests/unit_motif_ref.py, written from the definitions of include/mtr_hip.h -
the minimum over all 2p rotations of a unit and its reverse complement, the smallest divisor, a dict aggregation - applied to crafted
units (mtr_test_unit_motifs runs the product's kernels on them) and to the units, copies and lengths the reference's recorded stdout
prints for the golden cases."""
import ctypes as C
import os

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu
from tests import unit_motif_ref as ref
from tests.test_gpu_report import _golden_reads

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _check_units(eng, units, read=None, copies=None, repeat_len=None, table_slots=0, what=""):
    n = len(units)
    rd = np.arange(n) if read is None else np.asarray(read)
    cp = np.ones(n, np.int64) if copies is None else np.asarray(copies)
    ln = np.array([len(u) for u in units]) if repeat_len is None else np.asarray(repeat_len)
    got = eng.test_unit_motifs(units, read, copies, repeat_len, table_slots)
    ref.assert_catalogue(got, ref.catalogue(units, rd, cp, ln), what)
    return got


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- crafted units ----------------------------------------------------------------------------------------------------------------
def test_the_worked_values(eng):
    got = _check_units(eng, [u for u, *_ in ref.WORKED], what="worked values")
    motifs = got.motifs.tobytes()
    for k, (_, motif, strand, rotation, d) in enumerate(ref.WORKED):
        g = int(got.group[k])
        assert (motifs[got.motif_off[g]:got.motif_off[g + 1]], int(got.strand[k]), int(got.rotation[k]), int(got.motif_len[k])) == (motif, strand, rotation, d)
    assert got.group.tolist() == [0, 0, 1, 2, 3, 4, 4]                          # GT and ACAC are AC; CAG and CTG are AGC


def test_the_lengths_at_the_edges_of_the_paths(eng):
    rng = np.random.RandomState(31)
    units = [b""]
    for p in (1, 2, 63, 64, 65, 499, 500):
        units.append(bytes(b"ACGT"[c] for c in rng.randint(0, 4, size=p)))
        units.append(bytes(b"AC"[c] for c in rng.randint(0, 2, size=p)))
    units += [b"", b"T" * 499 + b"A", b"A" * 500, b"T" * 500]
    got = _check_units(eng, units, what="edge lengths")
    assert got.motif_len[0] == 0 and got.group[len(units) - 4] == got.group[0] and got.g_copies[got.group[0]] == 0      # the empty motif is a group too
    assert got.group[-1] == got.group[-2]                                        # A x 500 and T x 500 are the motif A


def test_non_primitive_units(eng):
    """no golden contains one: a unit that repeats a shorter root is this test's alone"""
    units = [b"ACAC", b"CA", b"GT", b"TGTGTG", b"CAGCAG", b"CTG", b"AAAA", b"T", b"ACGACGACG", b"GTC" * 100, b"AT" * 250, b"ATAT", b"TA",
             (b"A" * 249 + b"C") * 2, b"G" + b"T" * 249 + b"G" + b"T" * 249]
    copies = np.arange(3, 3 + len(units))
    got = _check_units(eng, units, copies=copies, what="non-primitive")
    assert got.motif_len.tolist() == [2, 2, 2, 2, 3, 3, 1, 1, 3, 3, 2, 2, 2, 250, 250]
    assert got.g_repeats.tolist() == [4, 2, 2, 2, 3, 2]
    assert got.g_copies[0] == 3 * 2 + 4 + 5 + 6 * 3                              # AC: ACAC counts twice its copies, TGTGTG three times


def test_three_hundred_random_units(eng):
    rng = np.random.RandomState(32)
    units = ref.random_units(rng, 300)
    units += [ref.rc(u) for u in units[:40]] + [u[7 % len(u):] + u[:7 % len(u)] for u in units[40:80]]         # some meet again on the other strand, or rotated
    n = len(units)
    read = np.sort(rng.randint(0, 60, size=n))
    got = _check_units(eng, units, read=read, copies=rng.randint(1, 2000, size=n), repeat_len=rng.randint(10, 100000, size=n), what="random units")
    assert len(got.g_first) < n - 40


# ---- group order and aggregation --------------------------------------------------------------------------------------------------
def test_group_order_and_aggregation(eng):
    roots = [b"CAG", b"AATGG", b"AC", b"TTAGGG", b"ACGT"]
    forms = []
    for m in roots:
        forms.append([m[r:] + m[:r] for r in range(len(m))] + [ref.rc(m)[r:] + ref.rc(m)[:r] for r in range(len(m))])
    units, pick = [], [3, 0, 1, 3, 2, 0, 4, 1]                                   # interleaved; motif 3 comes first, 4 last
    for k in range(40):
        m = pick[k % len(pick)]
        units.append(forms[m][(k * 5 + k // 8) % len(forms[m])])
    units[17] = units[17] * 4                                                      # a non-primitive member: four motifs per copy
    read = np.array([0] * 3 + [1] * 9 + [2] * 1 + [3] * 12 + [4] * 5 + [5] * 2 + [6] * 8)
    copies = 5 + np.arange(40) * 3
    repeat_len = 1000 + np.arange(40) * 17
    got = _check_units(eng, units, read=read, copies=copies, repeat_len=repeat_len, what="aggregation")
    assert got.g_first.tolist() == [0, 1, 2, 4, 6]
    assert got.group[:8].tolist() == [0, 1, 2, 0, 3, 1, 4, 2]
    assert got.g_repeats.tolist() == [10, 10, 10, 5, 5] and int(got.g_bases.sum()) == int(repeat_len.sum())
    assert got.motif_len[17] == len(units[17]) // 4 and all(got.g_reads <= 7) and any(got.g_reads < got.g_repeats)
    g17 = int(got.group[17])
    members = [k for k in range(40) if got.group[k] == g17]
    assert got.g_copies[g17] == sum(int(copies[k]) * (4 if k == 17 else 1) for k in members)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _distinct_motifs(rng, n, length=12):
    seen, out = set(), []
    while len(out) < n:
        u = bytes(b"ACGT"[c] for c in rng.randint(0, 4, size=length))
        m = ref.brute(u)[0]
        if m not in seen:
            seen.add(m)
            out.append(u)
    return out


def test_every_insert_contends_for_three_slots(eng):
    rng = np.random.RandomState(33)
    roots = [b"AGC", b"AAAAT", b"AACCCT"]
    units = []
    for k in range(4096):
        m = roots[int(rng.randint(0, 3))]
        s = m if rng.randint(0, 2) else ref.rc(m)
        r = int(rng.randint(0, len(s)))
        units.append((s[r:] + s[:r]) * int(rng.randint(1, 4)))
    read = np.sort(rng.randint(0, 500, size=4096))
    args = dict(read=read, copies=rng.randint(1, 50, size=4096), repeat_len=rng.randint(10, 5000, size=4096))
    a = _check_units(eng, units, what="4096 units of 3 motifs", **args)
    assert len(a.g_first) == 3 and int(a.g_repeats.sum()) == 4096
    assert _same(a, eng.test_unit_motifs(units, **args))                           # and again: the same catalogue


def test_a_nearly_full_table(eng):
    rng = np.random.RandomState(34)
    units = _distinct_motifs(rng, 1000)
    a = _check_units(eng, units, table_slots=1024, what="1000 motifs in 1024 slots")
    assert len(a.g_first) == 1000 and a.group.tolist() == list(range(1000))
    assert _same(a, eng.test_unit_motifs(units, table_slots=1024))
    assert _same(a, eng.test_unit_motifs(units))                                   # the product's table size: the same catalogue
    # with duplicates: 600 motifs, 400 of them twice, still 1024 slots
    units2 = units[:600] + [ref.rc(u) for u in units[:400]]
    b = _check_units(eng, units2, table_slots=1024, what="600 motifs, 1000 units, 1024 slots")
    assert len(b.g_first) == 600 and _same(b, eng.test_unit_motifs(units2, table_slots=1024))


def test_motifs_that_share_a_start_slot(eng):
    """the start slot is a function of the motif alone (tests/test_unit_motif_host.py pins ref.start_slot to the header): in a table of 64
    slots, eight motifs that all start at one slot, their members interleaved - every one probes past the others"""
    rng = np.random.RandomState(35)
    pool = {}
    for u in _distinct_motifs(rng, 1200, length=9):
        pool.setdefault(ref.start_slot(ref.brute(u)[0], 64), []).append(u)
    slot, same = max(pool.items(), key=lambda kv: len(kv[1]))
    assert len(same) >= 8, "1200 motifs over 64 slots leave one with eight"
    same = same[:8]
    assert len({ref.start_slot(ref.brute(u)[0], 64) for u in same}) == 1
    units = [same[k % 8] if k % 3 else ref.rc(same[k % 8]) for k in range(48)]
    a = _check_units(eng, units, table_slots=64, what="eight motifs on one start slot")
    assert len(a.g_first) == 8 and a.g_repeats.tolist() == [6] * 8
    assert _same(a, eng.test_unit_motifs(units, table_slots=64))


def test_the_test_entry_refuses_what_it_says(eng):
    for units, kw in [([b"ACGN"], {}), ([b"A" * 501], {}), ([b"acgt"], {}), ([b"AC", b"AG"], dict(read=[1, 0])), ([b"AC"] * 4, dict(table_slots=4)),
                      ([b"AC"] * 4, dict(table_slots=24))]:
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
            eng.test_unit_motifs(units, **kw)
    got = eng.test_unit_motifs([])
    assert len(got.strand) == 0 and len(got.g_first) == 0 and got.motif_off.tolist() == [0]
    assert len(eng.test_unit_motifs([b"AC"] * 4, table_slots=8).g_first) == 1


# ---- the golden cases --------------------------------------------------------------------------------------------------------------
def _stdout_catalogue(name, ids):
    """the brute force's catalogue of the reference's recorded stdout: its unit, copies and length columns, the read by its ID"""
    lines = open(os.path.join(gu.GOLDEN, f"{name}.default.stdout"), "rb").read().split(b"\n")[:-1]
    cols = [ln.split(b"\t") for ln in lines]
    assert all(len(c) == 13 for c in cols) and len(set(ids)) == len(ids)
    bid = [i.encode() for i in ids]
    return ref.catalogue([c[12] for c in cols], [bid.index(c[0]) for c in cols], [int(c[6]) for c in cols], [int(c[4]) for c in cols])


def _as_motifs(cat):
    return mtr_amd.ReportMotifs(**cat)


@pytest.mark.parametrize("name", [n for n, _ in gu.cases("default")])
def test_golden_cases(eng, name):
    ids, reads, _ = _golden_reads(name)
    want = _stdout_catalogue(name, ids)
    eng.upload(reads)
    eng.run()
    mot = eng.report_motif_tensors()
    assert all(t.device.type == "cuda" for t in mot)
    ref.assert_catalogue(mot, want, name)
    if name == "worm_chrII_1":
        assert (mot.strand.numel(), mot.g_first.numel()) == (113, 44)
        assert (int((mot.rotation != 0).sum()), int((mot.strand == 1).sum()), int((mot.g_repeats > 1).sum())) == (73, 38, 14)
    assert mtr_amd.format_motifs(mot) == mtr_amd.format_motifs(_as_motifs(want))
    rep = eng.report_tensors()                                                     # repeat k here is repeat k there
    assert rep.read.numel() == mot.strand.numel()
    units, off = rep.units.cpu().numpy().tobytes(), rep.unit_off.cpu().numpy()
    assert all(len(units[off[k]:off[k + 1]]) % int(d) == 0 for k, d in enumerate(mot.motif_len.cpu().numpy()) if d)


# ---- the protocol ------------------------------------------------------------------------------------------------------------------
def _sizes(e, dst=None):
    R, G, M = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    st = e.lib.mtr_report_motifs_device(e.h, C.byref(dst) if dst is not None else None, C.byref(R), C.byref(G), C.byref(M))
    return st, (R.value, G.value, M.value)


def test_protocol():
    e = mtr_amd.Engine()
    try:
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
            e.report_motif_tensors()
        assert _sizes(e)[0] == 2                                                   # MTR_ERR_BAD_ARG before any run
        reads = [c for _, c in synth.make_reads("headline2k", 200, 3)]
        e.upload(reads)
        assert _sizes(e)[0] == 2                                                   # uploaded, not run
        e.run()
        first = e.report_motif_tensors()                                           # the catalogue before anybody asked for the chains
        rep = e.report_tensors()
        e.upload(reads)
        e.run()
        rep2 = e.report_tensors()                                                  # a fresh run: the chains first, with the alignments and the text
        e.report_alignment_tensors()
        e.report_bytes([str(i) for i in range(len(reads))])
        second = e.report_motif_tensors()
        assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(rep.fields, rep2.fields)
        third = e.report_motif_tensors()                                           # kept: the same again
        assert all(torch.equal(a, b) for a, b in zip(first, third))
        # against the brute force over the report's own units
        units, off, f = rep.units.cpu().numpy().tobytes(), rep.unit_off.cpu().numpy(), rep.fields.cpu().numpy()
        R = rep.read.numel()
        want = ref.catalogue([units[off[k]:off[k + 1]] for k in range(R)], rep.read.cpu().numpy(), f[:, 4], f[:, 2])
        ref.assert_catalogue(first, want, "200 headline reads")
        G, M = len(want["g_first"]), len(want["motifs"])
        assert R > 100 and 1 < G < R
        # the size query
        assert _sizes(e) == (0, (R, G, M))
        # a capacity below its size: MTR_ERR_OVERFLOW, the sizes, nothing written
        cols = [torch.full((max(n, 1),), 0x5A, dtype=dt, device="cuda") for n, dt in
                [(R, torch.uint8), (R, torch.int32), (R, torch.int32), (R, torch.int32), (G + 1, torch.int64), (M, torch.uint8),
                 (G, torch.int32), (G, torch.int32), (G, torch.int32), (G, torch.int64), (G, torch.int64)]]
        before = [c.clone() for c in cols]
        torch.cuda.synchronize()
        ptrs = [c.data_ptr() for c in cols]
        for caps in [(R - 1, G, M), (R, G - 1, M), (R, G, M - 1), (0, 0, 0)]:
            assert _sizes(e, mtr_amd.CReportMotifDst(*ptrs, *caps)) == (5, (R, G, M)), caps
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(cols, before)), caps
        # a NULL column that would be written
        for missing in range(11):
            p = list(ptrs)
            p[missing] = None
            assert _sizes(e, mtr_amd.CReportMotifDst(*p, R, G, M)) == (2, (R, G, M)), missing
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(cols, before)), missing
        # exact capacities: written, and what report_motif_tensors returned
        assert _sizes(e, mtr_amd.CReportMotifDst(*ptrs, R, G, M)) == (0, (R, G, M))
        torch.cuda.synchronize()
        assert all(torch.equal(c[:t.numel()], t) for c, t in zip(cols, first))
        # the test entry point borrows the catalogue's buffers: the batch's catalogue is made again and is the same
        e.test_unit_motifs([b"ACGT", b"AC"])
        assert all(torch.equal(a, b) for a, b in zip(first, e.report_motif_tensors()))
        # a second run of another batch replaces the catalogue
        other = [c for _, c in synth.make_reads("headline2k", 60, 4)]
        e.upload(other)
        e.run()
        mot2, rep3 = e.report_motif_tensors(), e.report_tensors()
        units, off, f = rep3.units.cpu().numpy().tobytes(), rep3.unit_off.cpu().numpy(), rep3.fields.cpu().numpy()
        ref.assert_catalogue(mot2, ref.catalogue([units[off[k]:off[k + 1]] for k in range(rep3.read.numel())], rep3.read.cpu().numpy(), f[:, 4], f[:, 2]),
                             "the second batch")
        assert mot2.strand.numel() != R
        # a batch without repeats
        rng = np.random.RandomState(36)
        e.upload([rng.randint(0, 4, size=40).astype(np.uint8) for _ in range(8)])
        e.run()
        assert _sizes(e) == (0, (0, 0, 0))
        empty = e.report_motif_tensors()
        assert empty.motif_off.cpu().tolist() == [0] and all(t.numel() == 0 for i, t in enumerate(empty) if i != 4)
        assert _sizes(e, mtr_amd.CReportMotifDst(*([None] * 4), cols[4].data_ptr(), *([None] * 6), 0, 0, 0)) == (0, (0, 0, 0))
        assert _sizes(e, mtr_amd.CReportMotifDst(*([None] * 11), 0, 0, 0))[0] == 2  # motif_off is always written
        assert mtr_amd.format_motifs(empty) == b""
    finally:
        e.close()


# ---- a walk ------------------------------------------------------------------------------------------------------------------------
def test_a_walk_adds_up_to_the_one_batch_catalogue(eng):
    name = "synth_c4"
    data = open(gu.input_path(name), "rb").read()
    buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    eng.upload_fasta_device(buf)
    eng.run()
    whole = eng.report_motif_tensors()
    one = mtr_amd.MotifCatalog().add(whole)
    assert one.format() == mtr_amd.format_motifs(whole) and len(one) == 22
    cat, batches, seen = mtr_amd.MotifCatalog(), 0, []
    for fa in eng.walk_fasta_device(buf, len(data) // 5 + 1):
        if len(fa.lens):
            eng.run()
            mot = eng.report_motif_tensors()
            cat.add(mot)
            batches += 1
            seen += [r[0] for r in mtr_amd.MotifCatalog().add(mot).rows()]
    assert batches >= 3
    assert sorted(cat.rows()) == sorted(one.rows())
    assert [r[0] for r in cat.rows()] == list(dict.fromkeys(seen))                  # first appearance over the batches
    assert [r[0] for r in cat.rows()] == [r[0] for r in one.rows()]                 # which is first appearance in the file: the batches are in file order
