"""Three contexts in one process hold three DIFFERENT small batches and their chains overlap on the chip (GPU).

The kernels of one batch share CUs with those of another: a DP wavefront may run beside walk and range wavefronts of another context, and
mtr_k_revise_quads keeps no LDS arena - the votes of its tracebacks, and its fallbacks for units above 128 bases (revise_sub / dp_sub), use the wavefront's global
scratch.  Whatever shares a CU, every context's records are those of its batch run alone, and those are the oracle's."""
import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth

pytestmark = pytest.mark.gpu

MODE_VARS = ("MTR_STAGED", "MTR_QUAD_MIN", "MTR_TWO_PASS", "MTR_TEST_STAGED_CAPS", "MTR_TEST_STAGED_FLAGS")
MODES = {"staged_quads": {"MTR_STAGED": "1", "MTR_QUAD_MIN": "1"},
         "staged_two_pass_quads": {"MTR_STAGED": "1", "MTR_TWO_PASS": "1", "MTR_QUAD_MIN": "1"}}      # (the two-pass mode of tests/test_gpu_parity.py)
SEEDS = (311, 312, 313)


def _long_unit_batch():
    """2 reads with a unit of 200 bases x 6 copies (about 1.3 kb): above the 128 bases a pass of mtr_k_revise_quads takes, so their revisions run revise_sub / dp_sub"""
    rng = np.random.RandomState(4110)
    return [synth.make_read(rng, 200, 6, 50, 50)[0] for _ in range(2)]


@pytest.fixture(scope="module")
def batches():
    return [[c for _, c in synth.make_reads("headline2k", 48, seed)] for seed in SEEDS] + [_long_unit_batch()]


@pytest.fixture(scope="module")
def oracle_records(batches):
    """the CPU oracle's records of every batch, computed once and shared by both modes"""
    from tests.oracle_binding import Oracle
    orc = Oracle()
    want = [[orc.process(codes) for codes in reads] for reads in batches]
    orc.close()
    return want


def _records(e):
    return [[tuple(r) for r in g] for g in e.fetch()]


def _diff(i, want, got):
    return f"read {i}: {len(want)} records expected, {len(got)} produced; first difference {next(((a, b) for a, b in zip(want, got) if a != b), None)}"


@pytest.mark.parametrize("mode", sorted(MODES))
def test_overlapping_contexts_with_different_batches(monkeypatch, batches, oracle_records, mode):
    for k in MODE_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    # every batch alone on a fresh engine: the oracle's records
    alone = []
    for b, reads in enumerate(batches):
        e = mtr_amd.Engine()
        try:
            e.upload(reads)
            e.run()
            assert e.last_mode() == "staged chain" and e.counters()["reads_sent_back"] == 0, b
            alone.append(_records(e))
        finally:
            e.close()
        for i, want in enumerate(oracle_records[b]):
            assert alone[b][i] == want, f"batch {b} alone, " + _diff(i, want, alone[b][i])
    assert any(len(g) > 0 for g in alone[3]), "the long-unit batch reports its repeat"
    # three at a time, launched back to back as the benchmark's step does (upload; run_async ... ; wait ...; fetch): the three headline batches, then two of them
    # around the long-unit batch
    for trio in ((0, 1, 2), (0, 3, 2)):
        engines = [mtr_amd.Engine() for _ in trio]
        try:
            for e, b in zip(engines, trio):
                e.upload(batches[b])
            for e in engines:
                e.run_async()
            for e in engines:
                e.wait()
            for e, b in zip(engines, trio):
                assert e.last_mode() == "staged chain" and e.counters()["reads_sent_back"] == 0, b
                got = _records(e)
                for i, want in enumerate(alone[b]):
                    assert got[i] == want, f"batch {b} beside {trio}, " + _diff(i, want, got[i])
        finally:
            for e in engines:
                e.close()
