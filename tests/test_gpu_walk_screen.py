"""The dead-range screen in front of the walks (mtr_k_walk_screen, mtr_amd/csrc/k3_staged.hip.inc) on the GPU: one batch - the crafted reads of
tests/walk_screen_cases.py (short repeats at the rule's threshold, windows at a read's end), six headline reads, two reads whose widest window has
w >= 1 280 (ranges the rule must leave alone) - through the staged chain with the screen and with MTR_TEST_WALK_SCREEN=0.  The wire bytes must be
the same and the oracle's, and every counter that is a function of the batch must keep its value: a screened range counts what its wavefront counted."""
import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import host_util as hu
from tests import walk_screen_cases as cases
from tests.oracle_binding import Oracle
from tests.test_gpu_parity import MODE_VARS, MODES

pytestmark = pytest.mark.gpu

# One counter is no function of the batch: the bytes of cell matrix a four-per-wavefront alignment pass writes run to the longest of the alignments
# that happen to share it, and which ones do follows the order in which wavefronts append to the chain's lists - free with and without the screen.
# Measured: four runs of ONE arrangement give four values of it, screen off (10 265 472 .. 10 267 136 on this batch's like) and on, and no other
# counter differs (profiles/README.md).  The cells of those passes (qpass_cells_dp2) are compared like every other counter.
ORDER_DEPENDENT = ("qpass_bytes_dp2",)
SCREEN_MODES = ("staged", "staged_quads", "staged_two_pass", "staged_two_pass_all_wide_first")


@pytest.fixture(scope="module")
def batch():
    """-> (reads, the oracle's records of every read in the wire form)"""
    long_reads = cases.long_reads()
    reads = [codes for _, codes, _ in cases.crafted()] + [c for _, c in synth.make_reads("headline2k", 6, 2)] + long_reads
    orc = Oracle()
    try:
        for codes in long_reads:
            assert len(codes) >= 2600 and max(w for _, _, w, _ in orc.ranges(codes)) >= 1280
        want = b"".join(hu.wire_record(r) for codes in reads for r in orc.process(codes))
    finally:
        orc.close()
    assert len(reads) >= 10
    return reads, want


def _run(monkeypatch, reads, env, screen):
    for k in MODE_VARS + ("MTR_TEST_WALK_SCREEN",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not screen:
        monkeypatch.setenv("MTR_TEST_WALK_SCREEN", "0")
    e = mtr_amd.Engine()
    try:
        e.upload(reads)
        e.run()
        data, counts = e.fetch_packed()
        return data, counts.tolist(), e.counters(), e.last_mode()
    finally:
        e.close()


@pytest.mark.parametrize("mode", SCREEN_MODES)
def test_screen_on_and_off_give_the_same_bytes_and_counters(monkeypatch, batch, mode):
    reads, want = batch
    on = _run(monkeypatch, reads, MODES[mode], True)
    off = _run(monkeypatch, reads, MODES[mode], False)
    assert on[3] == "staged chain" and off[3] == "staged chain"
    assert on[1] == off[1] and on[0] == off[0]
    assert on[0] == want
    c_on, c_off = ({k: v for k, v in c.items() if k not in ORDER_DEPENDENT} for c in (on[2], off[2]))
    assert c_on == c_off, {k: (c_on[k], c_off[k]) for k in c_on if c_on[k] != c_off[k]}
    assert len(c_on) == len(on[2]) - len(ORDER_DEPENDENT)
    assert on[2]["reads_sent_back"] == 0 and on[2]["ranges_searched"] > 0 and on[2]["tables_skipped"] > 0


def test_a_full_survivor_list_sends_the_batch_to_the_per_read_kernel(monkeypatch, batch):
    reads, want = batch
    data, _, _, mode = _run(monkeypatch, reads, {"MTR_STAGED": "1", "MTR_TEST_STAGED_CAPS": "walk=3"}, True)
    assert mode == "per-read kernel"
    assert data == want
    # the same capacity with the screen off is not looked at: the chain keeps the batch
    data, _, _, mode = _run(monkeypatch, reads, {"MTR_STAGED": "1", "MTR_TEST_STAGED_CAPS": "walk=3"}, False)
    assert mode == "staged chain" and data == want
