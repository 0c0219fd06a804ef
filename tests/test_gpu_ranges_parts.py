"""The three-kernel range finder (launch_k1_parts: what the staged chain runs on a batch of at most 256 reads, i.e. on the long reads of a
command-line run) held to the oracle's ranges - run on the MI355X box with -m gpu.

Engine.test_ranges(finder="parts") runs it alone (mtr_test_ranges_parts) and returns every read's de-duplicated list: start, end, w and the
64 bits of the DI value.  Everything is compared exactly, in both DI modes, on the reads of tests/range_cases.py (what each of them is there
for is asserted on the CPU in tests/test_range_cases_ref.py): against the oracle, against the one-wavefront-per-read finder on the same
resident batch, across batch order and company, in file-order mode (the K1_FINISH form without segments), on the reference's G1 vectors.
"""
import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu
from tests import range_cases as rc
from tests.oracle_binding import Oracle

pytestmark = pytest.mark.gpu

MODES = [True, False]                      # Manhattan (Engine()), Pearson (Engine(manhattan=False))
BATCHES = list(rc.batches())


@pytest.fixture(scope="module")
def engines():
    e = {True: mtr_amd.Engine(), False: mtr_amd.Engine(manhattan=False)}
    yield e
    for x in e.values():
        x.close()


@pytest.fixture(scope="module")
def want():
    """(manhattan, case name) -> the oracle's ranges; computed once"""
    out = {}
    for m in MODES:
        o = Oracle(m)
        for name, c in rc.cases().items():
            out[m, name] = o.ranges(c.codes)
        o.close()
    return out


@pytest.fixture(scope="module")
def runs(engines):
    """(manhattan, batch name) -> (parts, wave): both finders on ONE resident batch; computed once per batch and mode"""
    done = {}

    def get(manhattan, batch):
        if (manhattan, batch) not in done:
            e = engines[manhattan]
            e.upload([rc.cases()[n].codes for n in rc.batches()[batch]])
            parts = e.test_ranges(finder="parts")
            done[manhattan, batch] = (parts, e.test_ranges(finder="wave"))
        return done[manhattan, batch]
    return get


def _first_difference(what, L, want, got):
    """names the read, its length and the first range that differs"""
    for t, (a, b) in enumerate(zip(want, got)):
        if tuple(a) != tuple(b):
            return f"{what} (L={L}): range {t} expected (start, end, w, DI bits) = {tuple(a)}, got {tuple(b)}"
    t = min(len(want), len(got))
    extra = f"first missing range {tuple(want[t])}" if len(want) > len(got) else f"first extra range {tuple(got[t])}"
    return f"{what} (L={L}): {len(want)} ranges expected, {len(got)} produced, the first {t} equal; {extra}"


def _assert_same(what, L, want, got):
    assert [tuple(x) for x in got] == [tuple(x) for x in want], _first_difference(what, L, want, got)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("manhattan", MODES)
def test_parts_ranges_equal_the_oracle(runs, want, manhattan, batch):
    parts, _ = runs(manhattan, batch)
    names = rc.batches()[batch]
    assert len(parts) == len(names)
    for i, name in enumerate(names):
        _assert_same(f"read {i} ({name}) of batch {batch}", rc.cases()[name].L, want[manhattan, name], parts[i])


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("manhattan", MODES)
def test_parts_ranges_equal_the_wave_finder_on_the_same_batch(runs, manhattan, batch):
    parts, wave = runs(manhattan, batch)
    for i, name in enumerate(rc.batches()[batch]):
        _assert_same(f"read {i} ({name}) of batch {batch}, against finder='wave'", rc.cases()[name].L, wave[i], parts[i])


@pytest.mark.parametrize("manhattan", MODES)
def test_ranges_do_not_depend_on_batch_order_or_company(runs, manhattan):
    fwd, rev, single = runs(manhattan, "mixed")[0], runs(manhattan, "mixed_reversed")[0], runs(manhattan, "single")[0]
    names = rc.batches()["mixed"]
    for i, name in enumerate(names):
        _assert_same(f"{name}: place {len(names) - 1 - i} of the reversed batch against place {i} of the mixed one", rc.cases()[name].L, fwd[i], rev[len(names) - 1 - i])
    alone = rc.batches()["single"][0]
    _assert_same(f"{alone}: alone against inside the mixed batch", rc.cases()[alone].L, fwd[names.index(alone)], single[0])


@pytest.mark.parametrize("manhattan", MODES)
def test_file_order_mode_takes_the_finish_without_segments(engines, manhattan):
    """a batch uploaded with a FileState: whole passes and mtr_k1_part(K1_FINISH); the oracle in file-order mode is the reference's behaviour on a file"""
    from tests.test_gpu_parity import _file_order_case
    reads = _file_order_case()
    assert len(reads) <= rc.PARTS_MAX
    o = Oracle(manhattan)
    o.set_file_order(True)
    expect = [o.ranges(c) for c in reads]
    o.close()
    e = engines[manhattan]
    fs = mtr_amd.FileState()
    try:
        e.upload(reads, fs)
        first = e.test_ranges(finder="parts")
        second = e.test_ranges(finder="parts")
    finally:
        fs.close()
    for i, c in enumerate(reads):
        _assert_same(f"read {i} of the file", len(c), expect[i], first[i])
        _assert_same(f"read {i} of the file, second call on the same resident batch", len(c), first[i], second[i])
    iso = Oracle(manhattan)
    differ = sum(1 for i, c in enumerate(reads) if iso.ranges(c) != expect[i])
    iso.close()
    assert differ >= 1                                    # (oracle against oracle: the stale tails change the ranges of this file, so the comparison above can fail)


@pytest.mark.parametrize("name,mode", gu.cases())
def test_parts_ranges_match_reference_golden(engines, name, mode):
    e = engines[mode == "default"]
    reads = [c for _, c in gu.read_fasta(gu.input_path(name))]
    cap = gu.capture_by_read(name, mode)
    assert len(cap) == len(reads)
    for lo in range(0, len(reads), rc.PARTS_MAX):
        e.upload(reads[lo:lo + rc.PARTS_MAX])
        got = e.test_ranges(finder="parts")
        for i, g in enumerate(got):
            _assert_same(f"read {lo + i} of {name} [{mode}]", len(reads[lo + i]), gu.g1_usable(cap[lo + i]["G1"]), g)


def _small_batch():
    reads = [c for _, c in synth.make_reads("c2", 8, 5)]
    reads.append(np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 80))
    return reads


def test_refusals_name_their_reason_and_leave_the_context_usable(monkeypatch, want):
    e = mtr_amd.Engine()
    try:
        with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: .*no batch uploaded"):
            e.test_ranges(finder="parts")
        good = rc.cases()["repeat_u7_4100"]
        e.upload([good.codes])
        _assert_same("after the refusal without a batch", good.L, want[True, "repeat_u7_4100"], e.test_ranges(finder="parts")[0])
        rng = np.random.RandomState(3)
        e.upload([rng.randint(0, 4, size=40).astype(np.uint8) for _ in range(rc.PARTS_MAX + 1)])
        with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: .*257 reads.*at most 256"):
            e.test_ranges(finder="parts")
        assert len(e.test_ranges(finder="wave")) == rc.PARTS_MAX + 1           # (the other finder takes the batch)
        e.upload([good.codes])
        _assert_same("after the refusal of 257 reads", good.L, want[True, "repeat_u7_4100"], e.test_ranges(finder="parts")[0])
        # per-read scratch for every read does not fit the context's budget: the chain would hand the batch to the other arrangement
        e.upload([good.codes, good.codes])
        monkeypatch.setenv("MTR_SCRATCH_MAX_GB", "0")
        with pytest.raises(mtr_amd.MtrError, match=r"MTR_ERR_BAD_ARG: .*scratch.*does not fit"):
            e.test_ranges(finder="parts")
        monkeypatch.delenv("MTR_SCRATCH_MAX_GB")
        both = e.test_ranges(finder="parts")
        _assert_same("after the refusal for scratch", good.L, want[True, "repeat_u7_4100"], both[1])
        with pytest.raises(ValueError):
            e.test_ranges(finder="neither")
    finally:
        e.close()


@pytest.mark.parametrize("manhattan", MODES)
def test_the_batch_still_runs_after_the_entry(engines, manhattan):
    reads = _small_batch()
    o = Oracle(manhattan)
    expect = [o.process(c) for c in reads]
    ranges = [o.ranges(c) for c in reads]
    o.close()
    e = engines[manhattan]
    e.upload(reads)
    got_ranges = e.test_ranges(finder="parts")
    e.run()
    got = e.fetch()
    for i, c in enumerate(reads):
        _assert_same(f"read {i}", len(c), ranges[i], got_ranges[i])
        assert [tuple(r) for r in got[i]] == expect[i], f"read {i}: the records after mtr_test_ranges_parts differ from the oracle's"
    assert sum(len(x) for x in expect) > 0
