"""mTR's report on the device (mtr_report_device, Engine.report_tensors, the kernels of mtr_amd/csrc/chain.hip.inc) on the MI355X.

Truth is the product's own host chain: mtrh_chain of mtr_amd/host/libmtr_host.so (ctypes) over the records fetch() returns.  The
chain of every read must be its records index for index, and format_report of the device report must print what the reference
printed: the golden stdout files byte for byte, and the known answers of whole BASELINE batches (no command line involved)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu
from tests import host_util as hu
from tests.test_gpu_parity import _crowded

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    hu.build_host()
    lib = C.CDLL(os.path.join(hu.HOST, "libmtr_host.so"))
    lib.mtrh_chain.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.mtrh_chain.restype = C.c_int
    return lib


def host_chain(lib, heads) -> list:
    """mtrh_chain over records given as int32 headers [n, >= 14] (mtrh_rec = {h, unit, score}; only h is read)"""
    h = np.zeros((max(len(heads), 1), 14), np.int32)
    if len(heads):
        h[:len(heads)] = np.asarray(heads, np.int32)[:, :14]
    recs = np.zeros((len(h), 3), np.uint64)
    recs[:, 0] = h.ctypes.data + 56 * np.arange(len(h), dtype=np.uint64)
    out = np.zeros(len(h), np.int32)
    n = lib.mtrh_chain(recs.ctypes.data, len(heads), out.ctypes.data)
    return out[:n].tolist()


def heads_of(records) -> np.ndarray:
    return np.array([r[:13] + (0,) for r in records], np.int32).reshape(-1, 14)


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_p():
    e = mtr_amd.Engine(manhattan=False)
    yield e
    e.close()


def _check_against_host(lib, got_records, rep):
    """every read's chain (the record column) is mtrh_chain over its records; fields / units are those records'; returns the chains"""
    counts = rep.counts.numpy()
    assert len(counts) == len(got_records)
    record = rep.record.cpu().numpy()
    read = rep.read.cpu().numpy()
    fields = rep.fields.cpu().numpy()
    unit_off, units = rep.unit_off.cpu().numpy(), rep.units.cpu().numpy().tobytes()
    assert int(unit_off[-1]) == len(units) and len(record) == int(counts.sum())
    k = 0
    for i, recs in enumerate(got_records):
        want = host_chain(lib, heads_of(recs))
        c = int(counts[i])
        assert record[k:k + c].tolist() == want, f"read {i}: device chain {record[k:k + c].tolist()} != host {want} ({len(recs)} records)"
        assert (read[k:k + c] == i).all()
        for t, j in enumerate(want):
            assert fields[k + t, :13].tolist() == list(recs[j][:13]), (i, j)
            assert units[unit_off[k + t]:unit_off[k + t + 1]].decode() == recs[j].unit, (i, j)
        k += c
    return record


def _golden_reads(name):
    """(ids, codes) of the reads mTR reports: the FASTA's records up to its first empty one (the reference stops there)"""
    recs, hdr, seq = [], None, []
    with open(gu.input_path(name)) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if hdr is not None:
                    recs.append((hdr, "".join(seq)))
                hdr, seq = line[1:], []
            else:
                seq.append(line)
    if hdr is not None:
        recs.append((hdr, "".join(seq)))
    cut = next((i for i, (_, s) in enumerate(recs) if not s), len(recs))
    return [h for h, _ in recs[:cut]], [mtr_amd.codes_from_str(s) for _, s in recs[:cut]], cut < len(recs)


# no golden input holds an empty record today; a case that does is compared on the reads before it and must be named here
CASES_WITH_AN_EMPTY_RECORD = set()


@pytest.mark.parametrize("name,mode", gu.cases("default") + gu.cases("p"))
def test_golden_cases_print_the_reference_stdout(host, eng, eng_p, name, mode):
    e = eng if mode == "default" else eng_p
    ids, reads, cut = _golden_reads(name)
    assert cut == (name in CASES_WITH_AN_EMPTY_RECORD), name
    e.upload(reads)
    e.run()
    got = e.fetch()
    rep = e.report_tensors()
    _check_against_host(host, got, rep)
    want = open(os.path.join(gu.GOLDEN, f"{name}.{mode}.stdout"), "rb").read()
    assert mtr_amd.format_report(ids, [len(r) for r in reads], rep) == want


def _ascii_tensor(reads):
    text = np.concatenate([np.frombuffer(b"ACGT", np.uint8)[r] for r in reads])
    lens = np.array([len(r) for r in reads], np.int32)
    offs = np.zeros(len(reads), np.int64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    return torch.from_numpy(text).to("cuda:0"), offs, lens


KNOWN = [("headline2k", 10000, False), ("headline2k", 10000, True), ("c2", 1000, False), ("c4", 10000, False)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg,n,pearson", KNOWN, ids=[f"{c}_{n}{'_p' if p else ''}" for c, n, p in KNOWN])
def test_whole_batches_match_their_known_answers(eng, eng_p, cfg, n, pearson):
    """one batch each; format_report with IDs str(i) reproduces the stdout known answer (tests/golden/<cfg>_<n>[_p]_stdout.json, the
    reference run one read per process).  The default headline batch goes in as ASCII text in a torch tensor."""
    known = hu.load_known(f"{cfg}_{n}{'_p' if pearson else ''}_stdout.json")
    reads = [c for _, c in synth.make_reads(cfg, n, synth.CONFIGS[cfg][4])]
    e = eng_p if pearson else eng
    if cfg == "headline2k" and not pearson:
        e.upload_device(*_ascii_tensor(reads))
    else:
        e.upload(reads)
    e.run()
    rep = e.report_tensors()
    out = mtr_amd.format_report([str(i) for i in range(n)], [len(r) for r in reads], rep)
    assert (hashlib.sha256(out).hexdigest(), out.count(b"\n"), len(out)) == (known["sha256"], known["stdout_lines"], known["stdout_bytes"])


def test_a_read_with_more_records_than_slots(host, eng):
    """the crowded read of test_gpu_parity.py::test_more_records_than_slots: its records come from the overflow buffer (resolve_overflow)"""
    reads = [c for _, c in synth.make_reads("c2", 5, 77)] + [_crowded(31)] + [c for _, c in synth.make_reads("c2", 5, 78)]
    e = eng
    e.upload_packed(reads)
    e.run()
    got = e.fetch()
    assert len(got[5]) > 16 + max(len(r) for r in reads) // 100
    _check_against_host(host, got, e.report_tensors())


def test_a_read_of_the_maximum_length(host, eng):
    """more than 500 records: the chain's working arrays live in global scratch"""
    rng = np.random.RandomState(99)
    parts = []
    for unit_len, copies in ((180, 40), (3, 300), (60, 150)):
        parts.append(rng.randint(0, 4, size=270000).astype(np.uint8))
        parts.append(synth.make_read(rng, unit_len, copies, 0, 0)[0])
    read = np.concatenate(parts)
    read = np.concatenate([read, rng.randint(0, 4, size=mtr_amd.MAX_READ_LENGTH - len(read)).astype(np.uint8)])
    reads = [read] + [c for _, c in synth.make_reads("c2", 3, 5)]
    eng.upload(reads)
    eng.run()
    got = eng.fetch()
    assert len(got[0]) > 500
    _check_against_host(host, got, eng.report_tensors())


def test_chain_kernel_fuzz(host, eng):
    """mtr_test_chain (the same device function) on seeded sets from tiny ranges: ties of keys and of ends, end == start + 10 and the
    erase loop's skip are hit constantly; the LDS path, the 64-entry steps and global scratch all run"""
    rng = np.random.RandomState(2024)
    sizes = [0, 1, 2, 63, 64, 65, 128, 129] * 300 + [1000] * 20 + [5000] * 6
    rng.shuffle(sizes)
    sets = []
    for n in sizes:
        span = int(rng.choice([4, 16, max(8, n // 4), max(8, 2 * n)]))
        start = rng.randint(0, span, size=n)
        end = start + rng.choice([-3, 0, 9, 10, 10, 11, 12, 20, 35], size=n) + rng.randint(0, 3, size=n)
        matches = rng.randint(0, int(rng.choice([2, 6, 40])), size=n)
        sets.append((start.astype(np.int32), end.astype(np.int32), matches.astype(np.int32)))
    got = eng.test_chain(sets)
    assert len(got) == len(sets)
    bad = []
    for k, (s, e, m) in enumerate(sets):
        h = np.zeros((len(s), 14), np.int32)
        h[:, 0], h[:, 1], h[:, 5] = s, e, m
        if got[k] != host_chain(host, h):
            bad.append(k)
    assert not bad, f"{len(bad)} of {len(sets)} sets differ; first: set {bad[0]} of {len(sets[bad[0]][0])} records"
    assert eng.test_chain([]) == []


@pytest.mark.parametrize("name", ["mixed_lengths", "stale_org_base"])
def test_file_order_batches(host, eng, name):
    """file-order mode (FileState), the file in two batches: each batch's report is mtrh_chain of that batch's records"""
    reads = [c for _, c in gu.read_fasta(os.path.join(gu.GOLDEN, "file_order", name + ".fa"))]
    fs = mtr_amd.FileState()
    try:
        half = max(1, len(reads) // 2)
        for part in (reads[:half], reads[half:]):
            if not part:
                continue
            got = eng.process_in_file(part, fs)
            _check_against_host(host, got, eng.report_tensors())
    finally:
        fs.close()


def test_protocol(host):
    e = mtr_amd.Engine()
    try:
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG"):
            e.report_tensors()
        reads = [c for _, c in synth.make_reads("headline2k", 200, 3)]
        e.upload(reads)
        e.run()
        got = e.fetch()
        counts = np.zeros(len(reads), np.int32)
        R, U = C.c_int64(), C.c_int64()
        assert e.lib.mtr_report_device(e.h, None, counts.ctypes.data, C.byref(R), C.byref(U)) == 0
        want = [host_chain(host, heads_of(g)) for g in got]
        assert counts.tolist() == [len(w) for w in want] and R.value == sum(len(w) for w in want) > 0
        assert U.value == sum(len(got[i][j].unit) for i, w in enumerate(want) for j in w)
        small = mtr_amd.CReportDst(None, None, None, None, None, None, R.value - 1, U.value)
        counts2 = np.zeros_like(counts)
        R2, U2 = C.c_int64(), C.c_int64()
        assert e.lib.mtr_report_device(e.h, C.byref(small), counts2.ctypes.data, C.byref(R2), C.byref(U2)) == 5      # MTR_ERR_OVERFLOW
        assert (R2.value, U2.value) == (R.value, U.value) and counts2.tolist() == counts.tolist()
        small = mtr_amd.CReportDst(None, None, None, None, None, None, R.value, U.value - 1)
        assert e.lib.mtr_report_device(e.h, C.byref(small), counts2.ctypes.data, C.byref(R2), C.byref(U2)) == 5
        rep = e.report_tensors()                                      # still usable; the same report
        _check_against_host(host, got, rep)
        f = rep.fields.cpu().numpy()
        want_ratio = f[:, 5].astype(np.float32) / f[:, 2].astype(np.float32)
        assert np.array_equal(rep.ratio.cpu().numpy().view(np.uint32), want_ratio.view(np.uint32))
        assert rep.unit_off.dtype == torch.int64 and rep.fields.shape == (R.value, 14) and rep.read.device.type == "cuda"
        # a run of reads that report nothing: zero-length columns
        e.upload([np.zeros(100, np.uint8)])                        # a homopolymer: mTR reports nothing (edge.fa)
        e.run()
        empty = e.report_tensors()
        assert empty.counts.tolist() == [0] and empty.read.numel() == 0 and empty.unit_off.cpu().tolist() == [0] and empty.units.numel() == 0
    finally:
        e.close()
