"""The quality-weighted consensus' reference (tests/consensus_quality_ref.py) on the CPU: the two properties the header states, on the inputs of
tests/consensus_cases.py (`limit` is the host program's, tests/test_consensus_quality_host.py); the answers worked out on paper in
tests/consensus_quality_cases.py; the gap weights at every kind of boundary; and the conditions by which the seed of the FASTQ test was chosen."""
import numpy as np
import pytest

from tests import consensus_cases as cc
from tests import consensus_quality_cases as qc
from tests import consensus_quality_ref as qref
from tests import consensus_ref as ref

NAMES = sorted(n for n in cc.all_cases() if n != "limit")


def _has_empty_window(case, qual):
    return any(al is not None and (len(al[1]) == 0 or any(len(w) == 0 for w, _ in al[3])) for al in qref.alleles(case, qual))


@pytest.mark.parametrize("name", NAMES)
def test_cap_one_is_the_unweighted_consensus_whatever_the_qualities(name):
    case, want = cc.expected()[name]
    case, qual, got = qref.expected(name, 1)
    assert len(set(qual.tolist())) > 1 or len(qual) < 2
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_a_constant_quality_scales_the_votes_where_no_window_is_empty(name):
    case, want = cc.expected()[name]
    c = 7
    qual = np.full(len(case["win_bases"]), c, np.uint8)
    if _has_empty_window(case, qual):
        assert name in ("lengths", "empty_backbone", "empty_member")       # (the property is not claimed there: an empty window's gap weight is 1, not c)
        return
    got = qref.consensus(case, qual, case["band_extra"], 40)
    for k in (0, 1, 3, 4, 5, 6, 7):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert np.array_equal(got[2], c * want[2]), name


@pytest.mark.parametrize("name", sorted(qc.hand_cases()))
def test_the_answers_worked_out_on_paper(name):
    members, cap, (bases, votes), plain = qc.hand_cases()[name]
    case, qual = qc.hand_case_columns(members)
    got = qref.consensus(case, qual, 16, cap)
    assert got[1].tolist() == bases and got[2].tolist() == votes and got[0].tolist() == [0, len(bases), len(bases)]
    assert ref.consensus(case, 16)[1].tolist() == plain
    assert qref.consensus(case, qual, 16, 1)[1].tolist() == plain


def test_a_run_of_six_fills_four_slots_and_casts_no_end_vote():
    members = qc.hand_cases()["ins_six"][0]
    (B, _), (W, Q) = members
    votes = qref.member_votes(W, Q, B, 16, 40)
    assert [v for v in votes if v[0] == "ins"] == [("ins", 1, 0, qc.G, 40), ("ins", 1, 1, qc.T, 40), ("ins", 1, 2, qc.G, 40), ("ins", 1, 3, qc.T, 40)]
    assert [v for v in votes if v[0] == "end"] == [("end", 0, 0, 40), ("end", 2, 0, 40)]       # boundaries 0 and n of the member: the one base that exists
    assert qref.columns(W, B, 16) == [(0, 0, None), (1, 7, "diag"), (8, 8, "diag")]


def test_the_gap_weights_at_the_boundaries():
    assert [qref.gap([5, 9, 3], i) for i in range(4)] == [5, 5, 3, 3] and qref.gap([], 0) == 1 and qref.gap([8], 0) == qref.gap([8], 1) == 8
    assert [qref.weight(q, 40) for q in (0, 1, 2, 40, 41, 93)] == [1, 1, 2, 40, 40, 40] and qref.weight(0, 1) == qref.weight(60, 1) == 1
    # a deletion before the member's first base and behind its last: boundary 0 and boundary n of a one-base window
    assert ("del", 1, 7) in qref.member_votes([qc.A], [7], [qc.T, qc.A], 16, 40)
    assert ("del", 2, 7) in qref.member_votes([qc.A], [7], [qc.A, qc.T], 16, 40)
    # an empty member deletes everything with weight 1
    assert qref.member_votes([], [], [qc.C, qc.A], 16, 40) == [("end", 0, 0, 1), ("del", 1, 1), ("end", 1, 0, 1), ("del", 2, 1), ("end", 2, 0, 1)]


def test_the_fastq_seed_does_what_it_was_chosen_for():
    assert qc.fq_seed_is_good(qc.FQ_SEED)
    reads = qc.fq_reads()
    text = qc.fastq_bytes(reads).split(b"\n")
    assert len(text) == 4 * len(reads) + 1 and text[0] == b"@r0" and len(text[1]) == len(text[3]) == len(reads[0][0]) and text[2] == b"+"
    case, qual = qc.fq_case()
    assert len(qual) == len(case["win_bases"]) and int(qual.min()) >= 2 and int(qual.max()) <= 39
