"""The reference of the window edits (tests/window_edits_ref.py) against windows worked out by hand from include/mtr_hip.h's definition ("window
edits"), the two invariants, and its per-window columns against the window structure's reference on every input of
tests/window_structure_cases.py (CPU)."""
import numpy as np
import pytest

from tests import window_edits_cases as ec
from tests import window_edits_ref as ref
from tests import window_structure_cases as wc
from tests import window_structure_ref as ws_ref

A, C, G, T = 0, 1, 2, 3
SUB, INS, DEL = 0, 1, 2

# (what it shows, structure, window, score, edits [pos, segment, copy, column, kind, base], the used segments' (start, end, copies, matches)[, scores])
HAND = [
    ("one substitution in a middle copy", ["CAG"], "CAGCAG" + "CTG" + "CAGCAG", 13, [[7, 0, 2, 1, SUB, T]], [(0, 15, 5, 14)]),
    ("one insertion in a middle copy", ["CAG"], "CAGCAG" + "CATG" + "CAG", 11, [[8, 0, 2, 1, INS, T]], [(0, 13, 4, 12)]),
    ("one deletion in a middle copy", ["CAG"], "CAGCAG" + "CG" + "CAG", 10, [[7, 0, 2, 1, DEL, A]], [(0, 11, 4, 11)]),
    ("an edit in copy 0 and one in the last copy", ["CAG"], "CTG" + "CAGCAG" + "CAA", 8, [[1, 0, 0, 1, SUB, T], [11, 0, 3, 2, SUB, A]], [(0, 12, 4, 10)]),
    ("an edit at first(s)", ["CAG"], "CAG" + "TAG" + "CAG", 7, [[3, 0, 1, 0, SUB, T]], [(0, 9, 3, 8)]),
    ("an edit at last(s)", ["CAG"], "CAG" + "CAT" + "CAG", 7, [[5, 0, 1, 2, SUB, T]], [(0, 9, 3, 8)]),
    ("an up step on a last column: the copy index does not advance", ["CAG"], "CAG" + "CAGT" + "CAG", 8, [[6, 0, 1, 2, INS, T]], [(0, 10, 3, 9)]),
    ("the wrap's left", ["CAG"], "CAGCAG" + "AG" + "CAG", 10, [[6, 0, 2, 0, DEL, C]], [(0, 11, 4, 11)]),
    ("the wrap's left and its run-on", ["CAG"], "CAGCAG" + "G" + "CAG", 48, [[6, 0, 2, 0, DEL, C], [6, 0, 2, 1, DEL, A]], [(0, 10, 4, 10)], (5, 1, 1)),
    ("at (1, 1, 1) that G is an insertion: the up ties the run-on's left and comes first", ["CAG"], "CAGCAG" + "G" + "CAG", 8, [[5, 0, 1, 1, INS, G]], [(0, 10, 3, 9)]),
    ("an entry by left in row 0", ["CAG"], "AG" + "CAG", 4, [[0, 0, 0, 0, DEL, C]], [(0, 5, 2, 5)]),
    ("a skipped segment", ["CAG", "CCG"], "CCG" + "CTG", 4, [[4, 1, 1, 1, SUB, T]], [(0, 0, 0, 0), (0, 6, 2, 5)]),
    ("the copy index counts within the segment", ["CAG", "CCG"], "CAGCAG" + "CCG" + "CTG" + "CCG", 13, [[10, 1, 1, 1, SUB, T]], [(0, 6, 2, 6), (6, 15, 3, 8)]),
    ("START as the end", ["CAG", "CCG"], "TT", -2, [], [(2, 2, 0, 0), (2, 2, 0, 0)]),
    ("the rows spent in START are no edits", ["CAG"], "TT" + "CAGCAG", 4, [], [(2, 8, 2, 6)]),
    ("(CAG)10 CAA (CAG)9", ["CAG"], "CAG" * 10 + "CAA" + "CAG" * 9, 58, [[32, 0, 10, 2, SUB, A]], [(0, 60, 20, 59)]),
    ("an empty window", ["CAG"], "", 0, [], [(0, 0, 0, 0)]),
]


@pytest.mark.parametrize("hand", HAND, ids=[h[0] for h in HAND])
def test_hand_worked_windows(hand):
    what, structure, window, score, edits, segs = hand[:6]
    got = ref.edits(structure, window, *(hand[6] if len(hand) > 6 else (1, 1, 1)))
    assert got.score == score and got.edits == edits and got.seg[:len(structure)] == [list(s) for s in segs] and got.skipped == 0, (what, got)
    assert ref.invariants_hold(structure, got), what


def test_the_hand_worked_steps_are_the_ones_named():
    """the windows above take the steps they are there for"""
    by = {h[0]: ref.edits(h[1], h[2], *(h[6] if len(h) > 6 else (1, 1, 1))).path for h in HAND}
    assert (6, 0, "left", 2) in by["the wrap's left"]                                        # first(0) from last(0) in its own row
    assert [(6, 0, "left", 2), (6, 1, "left", 0)] == by["the wrap's left and its run-on"][6:8]
    assert by["an entry by left in row 0"][0] == (0, 0, "left", ref.START)
    assert (7, 2, "up", 2) in by["an up step on a last column: the copy index does not advance"]
    assert by["START as the end"] == []


def test_a_window_beyond_the_limit_is_skipped_and_has_no_edits():
    got = ref.edits(["A"], np.zeros(ref.MAX_WINDOW + 1, np.uint8))
    assert got.skipped == 1 and got.edits == [] and got.score == 0 and got.seg == [[0] * 4] * 4


@pytest.mark.parametrize("scores", wc.SCORES)
def test_seg_and_score_are_the_window_structures_and_the_invariants_hold(scores):
    kinds = set()
    for name, case in ec.all_cases().items():
        for w, k in zip(case["windows"], case["which"]):
            st = case["structures"][k]
            got, want = ref.edits(st, w, *scores), ws_ref.structure(st, w, *scores)
            assert got.seg == want.seg and got.score == want.score and got.skipped == want.skipped, (name, st, w)
            assert ref.invariants_hold(st, got), (name, st, w)
            kinds |= {row[4] for row in got.edits}
    assert kinds == {SUB, INS, DEL}
