"""File-order mode for reads that are already in device memory, on the MI355X: Engine.upload_device / process_device /
upload_fasta_device with a FileState, FileState.skip_device (mtr_upload_batch_device_in_file, mtr_upload_fasta_device_in_file,
mtr_file_state_skip_device, the kernels of mtr_amd/csrc/file_order.hip.inc).  The yardstick is the host path - Engine.upload(reads,
FileState()) / process_in_file, pinned to the reference by tests/test_gpu_parity.py and tests/golden/file_order/ - and those goldens
themselves."""
import gzip
import json
import os

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
FO = os.path.join(gu.GOLDEN, "file_order")


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _plan(reads):
    lens = np.array([len(r) for r in reads], np.int32)
    return (np.cumsum(lens, dtype=np.int64) - lens), lens


def _ascii(reads):
    """(text tensor of 'ACGT' bytes on the GPU, offsets, lens) of reads given as codes"""
    offs, lens = _plan(reads)
    return torch.from_numpy(ACGT[np.concatenate(reads)]).cuda(), offs, lens


def _codes(reads):
    offs, lens = _plan(reads)
    return torch.from_numpy(np.concatenate(reads).astype(np.uint8)).cuda(), offs, lens


def _rec(per_read):
    return [[tuple(r) for r in rs] for rs in per_read]


# ---- 1: the tail kernel and the after-bases kernel alone (upload only, no run) -----------------------------------------------------
# One file; by mtr_file_state::walk a reader of 600 has E = 1000 and reach = 1028.  Behind 12000 its tail is that read's leading
# flank, behind 10100 it straddles r_e = 1010, behind 2000 it is own bases, behind 910 own bases run into the trailing flank inside a
# 5-mer, behind 820 it crosses the n_e - 4 switch from 5-mer to raw, behind 610 (E = 1010) it is mt[q] beyond n_e and then 900's
# entries: two owners.  999 / 1000: r = 100 / L/10.  720000: N capped at 1e6, owner of 60000's tail and of later leading flanks, and
# itself a long read with an empty tail that nothing precedes.  After-bases: owners of length L + 1 and L + 2 (615 behind 616 and 617;
# 599 behind 600 and 601), L and L + 1 in one word (910 % 16 = 14), L % 16 = 0 (2000), the second 600 behind 2000 only, 599 last.
# No length of that file has L % 16 = 15 (615 % 16 is 7), so WORD_EDGE_LENS adds the case where L and L + 1 fall in two words: 639 behind
# 640 and 641 (and 31, 15: a read shorter than one word).
TAIL_LENS = [720000, 60000, 12000, 10100, 600, 2000, 600, 910, 600, 820, 600, 1000, 600, 999, 600, 900, 610, 600, 617, 616, 615, 614,
             601, 600, 599]
WORD_EDGE_LENS = [2000, 641, 640, 639, 31, 15]
TAIL_CASES = {"one_batch": (TAIL_LENS, [(0, len(TAIL_LENS))]), "split": (TAIL_LENS, [(0, 1), (1, 5), (5, len(TAIL_LENS))]),
              "word_edges": (WORD_EDGE_LENS, [(0, 2), (2, len(WORD_EDGE_LENS))])}


@pytest.fixture(scope="module")
def tail_reads():
    rng = np.random.RandomState(20240917)
    return {id(lens): [rng.randint(0, 4, size=n).astype(np.uint8) for n in lens] for lens in (TAIL_LENS, WORD_EDGE_LENS)}


@pytest.fixture(scope="module")
def tail_want(eng, tail_reads):
    """per split, per batch: test_file_tail() after the host upload on a host state"""
    out = {}
    for name, (lens, cuts) in TAIL_CASES.items():
        fs = mtr_amd.FileState()
        out[name] = []
        for lo, hi in cuts:
            eng.upload(tail_reads[id(lens)][lo:hi], fs)
            out[name].append(eng.test_file_tail())
        fs.close()
    return out


def _assert_tails_equal(got, want, what):
    for k, name in enumerate(("tail", "tail_off", "after")):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, name, got[k].shape, want[k].shape)
        bad = np.flatnonzero(got[k].ravel() != want[k].ravel())
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:8].tolist()} ({len(bad)} entries): got {got[k].ravel()[bad[:8]].tolist()}, want {want[k].ravel()[bad[:8]].tolist()}"


@pytest.mark.parametrize("codes", [False, True], ids=["ascii", "codes"])
@pytest.mark.parametrize("split", sorted(TAIL_CASES))
def test_tails_and_after_bases_equal_the_host_state(eng, tail_reads, tail_want, split, codes):
    fs = mtr_amd.FileState()
    case_lens, cuts = TAIL_CASES[split]
    for b, (lo, hi) in enumerate(cuts):
        text, offs, lens = (_codes if codes else _ascii)(tail_reads[id(case_lens)][lo:hi])
        eng.upload_device(text, offs, lens, codes=codes, file_state=fs)
        _assert_tails_equal(eng.test_file_tail(), tail_want[split][b], f"{split} batch {b}")
    fs.close()


def test_the_tail_case_covers_what_it_claims(eng, tail_reads, tail_want):
    """the yardstick itself: the lengths derived by hand, non-zero entries, and a difference from the isolated upload"""
    tail, off, after = tail_want["one_batch"][0]
    n = np.diff(off)
    assert off.dtype == np.int64 and tail.dtype == np.uint16 and after.shape == (len(TAIL_LENS), 2)
    assert n[0] == 0                                                     # nothing precedes the first read
    assert n[1] == 86488 - 84000 and n[2] == 23448 - 16800               # reach - E of 60000 and 12000
    assert all(n[i] == 28 for i, L in enumerate(TAIL_LENS) if L == 600)
    assert (tail > 3).any() and (tail <= 3).any() and tail.max() < 1024  # 5-mer codes and raw entries
    assert after.any() and not after[0].any()
    edge = tail_want["word_edges"][1][2]                                 # 640, 639, 31, 15: each has two longer reads before it
    assert edge.shape == (4, 2) and edge.any()
    text, offs, lens = _ascii(tail_reads[id(TAIL_LENS)])
    eng.upload_device(text, offs, lens)
    t0, o0, a0 = eng.test_file_tail()
    assert len(t0) == 0 and not o0.any() and o0.shape == off.shape and not a0.any() and a0.shape == after.shape


# ---- 2: records --------------------------------------------------------------------------------------------------------------------
def _records_case():
    """tests/test_gpu_parity.py's file-order case, rebuilt: widely mixed lengths + reads ending inside their repeat right after a longer read"""
    reads = [c for _, c in synth.make_mixed_file(150, 21)]
    rng = np.random.RandomState(5)
    for n in (3000, 9, 1200, 31, 4, 700):
        reads.append(rng.randint(0, 4, size=n).astype(np.uint8))
        reads.append(np.concatenate([rng.randint(0, 4, size=max(0, n // 3)).astype(np.uint8), np.tile(rng.randint(0, 4, size=7).astype(np.uint8), 40)]))
    return reads


@pytest.fixture(scope="module")
def records_case(eng):
    reads = _records_case()
    fs = mtr_amd.FileState()
    want = _rec(eng.process_in_file(reads, fs))
    fs.close()
    return reads, want, _rec(eng.process(reads))


@pytest.mark.parametrize("mode", ["default", "per_read"])
def test_records_equal_the_host_state_whatever_the_batches(monkeypatch, eng, records_case, mode):
    reads, want, iso = records_case
    if mode == "per_read":
        monkeypatch.setenv("MTR_STAGED", "0")
    fs = mtr_amd.FileState()
    got = []
    for lo, hi in ((0, 1), (1, 8), (8, 97), (97, len(reads))):
        got += _rec(eng.process_device(*_ascii(reads[lo:hi]), file_state=fs))
        assert mode != "per_read" or eng.last_mode() == "per-read kernel"
    fs.close()
    for i in range(len(reads)):
        assert got[i] == want[i], f"read {i} (L={len(reads[i])}): {len(want[i])} records expected, {len(got[i])} produced"
    assert sum(1 for i in range(len(reads)) if iso[i] != want[i]) >= 3


def test_a_shard_behind_skip_device(eng, records_case):
    reads, want, iso = records_case
    fs = mtr_amd.FileState()
    text, offs, lens = _ascii(reads[:60])
    eng.upload([reads[0]])                                               # a resident batch that the skip must leave alone
    fs.skip_device(eng, text, offs, lens)
    eng.run()
    assert eng.n_reads == 1 and _rec(eng.fetch()) == iso[:1]
    part = _rec(eng.process_device(*_codes(reads[60:110]), codes=True, file_state=fs))
    fs.close()
    for i in range(60, 110):
        assert part[i - 60] == want[i], f"read {i}"


# ---- 3: the goldens end to end: file bytes in, the reference's ranges, records and -a stdout out ------------------------------------
def _capture(name):
    per_read = []
    with gzip.open(os.path.join(FO, f"{name}.default.cap.jsonl.gz"), "rt") as fh:
        for line in fh:
            ev = json.loads(line)
            if ev["t"] == "G1":
                per_read.append({"G1": ev, "G4": []})
            elif ev["t"] == "G4":
                per_read[-1]["G4"].append(ev)
    return [(gu.g1_usable(p["G1"]), [gu.g4_tuple(ev) for ev in p["G4"]]) for p in per_read]


def _device_bytes(raw):
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()


@pytest.mark.parametrize("name", ["mixed_lengths", "stale_org_base"])
def test_golden_file_bytes_in(eng, name):
    raw = open(os.path.join(FO, name + ".fa"), "rb").read()
    want = _capture(name)
    fs = mtr_amd.FileState()
    fa = eng.upload_fasta_device(_device_bytes(raw), fs)
    assert fa.end == "eof" and len(fa.ids) == len(want)
    ranges = eng.test_ranges()
    eng.run()
    got = _rec(eng.fetch())
    for i in range(len(want)):
        assert ranges[i] == want[i][0], f"read {i}: ranges differ"
        assert got[i] == want[i][1], f"read {i}: records differ"
    if name == "stale_org_base":
        assert eng.report_bytes(fa.ids, alignments=True) == open(os.path.join(FO, "stale_org_base.a.stdout"), "rb").read()
    fs.close()
    # the same file in two calls, cut at a record boundary: the state carries over
    starts = [i + 1 for i in range(len(raw) - 1) if raw[i:i + 2] == b"\n>"]
    cut = starts[len(starts) // 2]
    fs = mtr_amd.FileState()
    two, ids = [], []
    for part in (raw[:cut], raw[cut:]):
        fa = eng.upload_fasta_device(_device_bytes(part), file_state=fs)
        eng.run()
        two += _rec(eng.fetch())
        ids += fa.ids
    fs.close()
    assert len(ids) == len(want) and two == [w[1] for w in want]


# ---- 4: state discipline -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_file():
    rng = np.random.RandomState(99)
    return [rng.randint(0, 4, size=n).astype(np.uint8) for n in (5000, 700, 1500, 650, 600, 649)]


def test_a_refused_upload_leaves_the_state_as_it_was(eng, small_file):
    reads = small_file
    fresh = mtr_amd.FileState()
    eng.upload_device(*_ascii(reads[:2]), file_state=fresh)
    eng.upload_device(*_ascii(reads[2:]), file_state=fresh)
    want = eng.test_file_tail()
    fresh.close()
    assert want[0].any() and want[2].any()

    fs = mtr_amd.FileState()
    eng.upload_device(*_ascii(reads[:2]), file_state=fs)
    text, offs, lens = _ascii([reads[2], reads[1], reads[0]])           # would pop both stairs and leave others, were it accepted
    text[int(offs[1]) + 5] = ord("N")
    with pytest.raises(mtr_amd.MtrError, match="read 1"):
        eng.upload_device(text, offs, lens, file_state=fs)
    with pytest.raises(mtr_amd.MtrError):
        fs.skip_device(eng, text, offs, lens)
    with pytest.raises(mtr_amd.MtrError, match="read 0: length"):       # a bad argument that only the library sees: a read past the limit
        eng._check(eng.lib.mtr_upload_batch_device_in_file(eng.h, fs.h, text.data_ptr(), text.numel(), offs.ctypes.data,
                                                           np.array([mtr_amd.MAX_READ_LENGTH + 1, 1, 1], np.int32).ctypes.data, 3, 0, None), "upload")
    eng.upload_device(*_ascii(reads[2:]), file_state=fs)
    _assert_tails_equal(eng.test_file_tail(), want, "after the refusals")
    fs.close()


def test_a_state_keeps_its_kind(eng, small_file):
    reads = small_file
    dev, host = mtr_amd.FileState(), mtr_amd.FileState()
    eng.upload_device(*_ascii(reads[:2]), file_state=dev)
    eng.upload(reads[:2], host)
    with pytest.raises(mtr_amd.MtrError, match="fed from device memory"):
        eng.upload(reads[2:], dev)
    with pytest.raises(mtr_amd.MtrError):
        dev.skip(reads[2:])
    with pytest.raises(mtr_amd.MtrError, match="fed from the host"):
        eng.upload_device(*_ascii(reads[2:]), file_state=host)
    with pytest.raises(mtr_amd.MtrError, match="fed from the host"):
        host.skip_device(eng, *_ascii(reads[2:]))
    # both are still usable by their own kind, and agree
    eng.upload(reads[2:], host)
    want = eng.test_file_tail()
    eng.upload_device(*_ascii(reads[2:]), file_state=dev)
    _assert_tails_equal(eng.test_file_tail(), want, "after the refused calls")
    assert want[0].any()
    dev.close(); host.close()


def test_without_a_state_nothing_changes(eng, records_case):
    reads, _, iso = records_case
    got = _rec(eng.process_device(*_ascii(reads[:40])))
    assert got == iso[:40]
    tail, off, after = eng.test_file_tail()
    assert len(tail) == 0 and not off.any() and not after.any()
