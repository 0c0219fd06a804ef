"""polish_repeat on the GPU (consensus.c:610-704; polish() of k2_units.hip.inc on polish_plan.h's plan over the flagged positions).

  1. One wavefront per call through the test entry mtr_test_polish: the crafted calls of tests/polish_cases.py (a flag at position 0, flags inside
     the first k - 1 positions, flags closer than k, alterations with step 0 and step 2, an output beyond MAX_PERIOD, period <= k, units of 6 .. 499
     bases, k = 2 .. 12: direct, packed and split tables) against the walk over every position on the host (tests/polish_plan_check.cpp), and the
     first 200 polish calls of the CPU oracle on headline2k reads (its G3p capture lines) against the oracle's polished units.
  2. One 24-read batch of headline2k through the per-read kernel and the staged chain (tests.test_gpu_parity.MODES): the records must be the
     oracle's.  The chain's polish kernel copies an unchanged unit from the candidate's slot to the revision's record and writes a changed one
     from the walk's output; no smaller shape has both.  The seed is one whose batch has polish calls that change the unit (asserted on the CPU
     oracle's capture; about one call in eight does)."""
import pytest

import mtr_amd
from tests import polish_cases as cases
from tests.test_gpu_parity import MODES, _diff_msg
from tests.test_polish_plan_host import polish as host_polish, pp  # noqa: F401  (pp: the host library's fixture)

pytestmark = pytest.mark.gpu

BATCH_SEED = 3


def test_crafted_calls_through_the_test_entry(pp):  # noqa: F811
    cc = cases.crafted()
    e = mtr_amd.Engine()
    e.upload([c["read"] for c in cc])
    got = e.test_polish([(i, c["rep_start"], c["rep_end"], c["k"], c["unit"], c["score"]) for i, c in enumerate(cc)])
    e.close()
    for c, g in zip(cc, got):
        want, _ = host_polish(pp, 1, cases.pack(c["read"]), len(c["read"]), c["rep_start"], c["rep_end"], c["k"], c["unit"], c["score"])
        assert g.tolist() == want.tolist(), (c["name"], len(g), len(want))


def test_the_first_200_polish_calls_of_the_headline_reads_equal_the_oracle():
    reads, calls = cases.oracle_g3p("headline2k", 300, 2)
    calls = calls[:200]
    n_reads = max(g["rd"] for g in calls) + 1
    e = mtr_amd.Engine()
    e.upload(reads[:n_reads])
    got = e.test_polish([(g["rd"], g["rep_start"], g["rep_end"], g["k"], g["unit"], g["score"]) for g in calls])
    e.close()
    changed = 0
    for i, (g, out) in enumerate(zip(calls, got)):
        assert out.tolist() == g["out"].tolist(), (i, g["rd"], g["rep_start"], g["rep_end"], g["k"], len(out), len(g["out"]))
        changed += g["out"].tolist() != g["unit"].tolist()
    assert changed >= 10, changed


@pytest.mark.parametrize("mode", ["per_read", "staged", "staged_quads"])
def test_a_24_read_batch_gives_the_oracle_records(monkeypatch, mode):
    from tests.oracle_binding import Oracle
    reads, calls = cases.oracle_g3p("headline2k", 24, BATCH_SEED)
    changed = sum(g["out"].tolist() != g["unit"].tolist() for g in calls)
    assert changed >= 3 and changed < len(calls) - 3, (changed, len(calls))      # both ways out of the polish kernel
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    e = mtr_amd.Engine()
    got = e.process(reads)
    if mode.startswith("staged"):
        assert e.last_mode() == "staged chain"
    e.close()
    orc = Oracle()
    for i, codes in enumerate(reads):
        want = orc.process(codes)
        assert [tuple(r) for r in got[i]] == want, _diff_msg(i, want, [tuple(r) for r in got[i]])
    orc.close()
