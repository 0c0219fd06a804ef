"""The staged chain with its short-unit alignments eight per wavefront (-m gpu): one batch of a few hundred reads whose repeats have units of 1, 2, 8, 9,
16, 17, 32 and 33 bases - both sides of every eight-column border of the eight-lane pass, and the first length that stays four per wavefront - run above
quad_min in one pass and in two.  The record stream must equal the oracle's, and the pass counts (product builds: prof55 = passes of eight alignments,
prof47 = passes of four) must show that both kinds ran.
"""
import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth

pytestmark = pytest.mark.gpu

UNITS = (1, 2, 8, 9, 16, 17, 32, 33)
MODES = {"one_pass": {"MTR_STAGED": "1", "MTR_QUAD_MIN": "64", "MTR_TWO_PASS": "0"},
         "two_pass": {"MTR_STAGED": "1", "MTR_QUAD_MIN": "64", "MTR_TWO_PASS": "1"}}


def make_batch():
    """40 reads per unit length: 240 to 400 bases of repeat (few and many copies) between flanks of 0 to 120 bases, a tenth of them without errors"""
    rng = np.random.RandomState(20261)
    reads = []
    for u in UNITS:
        for i in range(40):
            copies = max(3, int(rng.randint(240, 401)) // u)
            pre, post = ((0, 120), (120, 0), (60, 60), (100, 100))[i % 4]
            reads.append(synth.make_read(rng, u, copies, pre, post, (0.0, 0.0, 0.0) if i % 10 == 9 else synth.NANOPORE)[0])
    return reads


@pytest.fixture(scope="module")
def batch():
    from tests.oracle_binding import Oracle
    reads = make_batch()
    orc = Oracle()
    want = [orc.process(r) for r in reads]
    orc.close()
    periods = {int(r[3]) for w in want for r in w}
    assert periods >= set(UNITS) - {1}, sorted(periods)       # (what the oracle reports; the alignments also see the search's other candidates)
    return reads, want


@pytest.mark.parametrize("mode", sorted(MODES))
def test_chain_with_eight_alignments_per_wavefront_matches_the_oracle(monkeypatch, batch, mode):
    reads, want = batch
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    e = mtr_amd.Engine()
    got = e.process(reads)
    assert e.last_mode() == "staged chain"
    cnt = e.counters()
    assert cnt["reads_sent_back"] == 0
    assert cnt["prof55"] > 50 and cnt["prof47"] > 0, (cnt["prof55"], cnt["prof47"])          # passes of eight, passes of four
    assert 0 < cnt["qpass_cells_dp2"] <= cnt["qpass_bytes_dp2"]          # a byte per served cell pair, and the padding
    for i, codes in enumerate(reads):
        assert [tuple(r) for r in got[i]] == want[i], f"read {i} (unit {UNITS[i // 40]}): want {want[i]} got {[tuple(r) for r in got[i]]}"
    e.close()
