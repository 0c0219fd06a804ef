"""tests/window_structure_ref.py (the window structure's definition in plain Python) held to answers worked out by hand, and the inputs of
tests/window_structure_cases.py shown not to be degenerate (CPU).  The reference notes what the walk back from the end met - every kind of
step, and the ties - so the small windows below prove that each rule of the definition decides at least one of these answers."""
import numpy as np
import pytest

from tests import window_structure_cases as wc
from tests import window_structure_ref as ref

# (window, structure, scores, score, the structure's segments, steps the walk must have taken), each short enough to follow with a pencil:
#   A / CAG           START -left-> C (row 0, entry 0: -1), A matches (0), -left-> G (-1): one copy; START(1) = -1 ties and comes later in the end's order
#   AA / CAG, G = 5   ... G of copy 1 is 3 in row 1; the wrap's left makes C 2, A matches (7), -left-> G: 6, two copies
#   GG / CAG, G = 5   START -left-> C -left-> A (-2), G matches (3): copy 1; the wrap's left (2) and its run-on to A (1), G matches: 6
#   AA / CAG, MM = 3  one copy as in the first line (-1), then the second A is an insertion: up (-2), which ties a left from A
#   AC / CAG CCG      G = 5: A in a copy of CAG entered and left by lefts (3), then -left-> C of CCG from outside (2), C matches (7), -left-> G: 6
#   AC / A C          two subs, the second from outside its segment: 2
#   CA / A C          C matches from START in segment 1 (1), A mismatches through the wrap (0): segment 0 skipped, a sub that ties up; the end ties
#                     last(0) = 0 (C inserted, A matched), and the higher segment wins
#   A / CAGT          a copy costs three lefts for one match: START (-1) is the end, both segments of nothing
STEPS = [
    ("A", ["CAG"], (1, 1, 1), -1, [[0, 1, 1, 1]], {"left:START", "left:row0-entry", "left:inside", "sub:inside", "end:tie"}),
    ("AA", ["CAG"], (5, 1, 1), 6, [[0, 2, 2, 2]], {"left:wrap", "left:START", "sub:inside"}),
    ("GG", ["CAG"], (5, 1, 1), 6, [[0, 2, 2, 2]], {"left:wrap", "left:run-on"}),
    ("AA", ["CAG"], (1, 3, 1), -2, [[0, 2, 1, 1]], {"up", "tie:up=left"}),
    ("AC", ["CAG", "CCG"], (5, 1, 1), 6, [[0, 1, 1, 1], [1, 2, 1, 1]], {"left:outside", "left:START"}),
    ("AC", ["A", "C"], (1, 1, 1), 2, [[0, 1, 1, 1], [1, 2, 1, 1]], {"sub:START", "sub:outside"}),
    ("CA", ["A", "C"], (1, 1, 1), 0, [[0, 0, 0, 0], [0, 2, 2, 1]], {"sub:wrap", "tie:sub=up", "end:tie"}),
    ("A", ["CAGT"], (1, 1, 1), -1, [[1, 1, 0, 0]], {"end:START"}),
]
KINDS = {"sub:START", "sub:inside", "sub:outside", "sub:wrap", "up", "left:START", "left:inside", "left:outside", "left:wrap", "left:run-on", "left:row0-entry",
         "tie:sub=up", "tie:up=left", "end:START", "end:tie"}


@pytest.mark.parametrize("window,st,scores,score,segs,steps", STEPS)
def test_small_windows_by_hand_and_the_rules_that_decide_them(window, st, scores, score, segs, steps):
    r = ref.structure(st, window, *scores)
    assert (r.score, r.seg[:len(st)], r.skipped) == (score, segs, 0) and r.seg[len(st):] == [[0] * 4] * (4 - len(st))
    assert steps <= r.steps, (steps - r.steps, r.steps)
    assert r.ratio == np.float32(sum(s[3] for s in segs)) / np.float32(len(window))


def test_every_kind_of_step_and_tie_is_taken_by_one_of_them():
    assert set().union(*(ref.structure(st, w, *sc).steps for w, st, sc, *_ in STEPS)) == KINDS


@pytest.mark.parametrize("window,st,scores,score,segs", wc.HAND)
def test_the_alleles_of_the_consensus_tests_and_the_edge_windows(window, st, scores, score, segs):
    r = ref.structure(st, window, *scores)
    assert r.score == score and r.seg[:len(st)] == [list(s) for s in segs], (r.score, r.seg)
    if window == "CAGCAGAGCAG":
        assert "left:wrap" in r.steps
    if window == "TT":
        assert "end:START" in r.steps


def test_the_limits():
    assert ref.limit_ok(["A" * 32]) and ref.limit_ok(["A" * 16, "C" * 16]) and ref.limit_ok(["ACGT"] * 4) and ref.limit_ok(["A" * 14, "C", "G"])
    assert not ref.limit_ok(["A" * 33]) and not ref.limit_ok(["A" * 16, "C" * 17]) and not ref.limit_ok(["A" * 15, "C", "G"]) and not ref.limit_ok(["A"] * 5)
    assert not ref.limit_ok([]) and not ref.limit_ok(["A", ""])
    long = ref.structure("A", np.zeros(ref.MAX_WINDOW + 1, np.uint8))
    assert long.skipped == 1 and long.score == 0 and long.seg == [[0] * 4] * 4
    empty = ref.structure(["CAG", "CCG"], "")
    assert (empty.score, empty.seg, float(empty.ratio), empty.skipped) == (0, [[0] * 4] * 4, 0.0, 0)


def test_the_cases_are_not_degenerate():
    cases = wc.all_cases()
    lanes = cases["lanes"]
    assert len(lanes["structures"]) == 130 and len({tuple(st) for st in lanes["structures"]}) == 130 and lanes["which"].tolist() == list(range(130))
    # a kernel that ran every lane with the structure of its wavefront's first lane would be wrong for almost every window
    (_, (seg, score, _, _)) = wc.expected()[("lanes", (1, 1, 1))]
    wrong = sum(1 for w in range(130) if ref.structure(lanes["structures"][64 * (w // 64)], lanes["windows"][w]).score != score[w])
    assert wrong > 100, wrong
    widths = cases["widths"]
    assert sorted({sum(len(m) for m in st) for st in widths["structures"] if len(st) <= 2}) == sorted(wc.WIDTHS_NARROW)
    assert sorted({(sum(len(m) for m in st), len(st)) for st in widths["structures"] if len(st) > 2}) == sorted((W, S) for W in wc.WIDTHS_WIDE for S in (3, 4))
    assert sorted({len(w) for w in widths["windows"]}) == sorted(wc.LENGTHS)
    assert {int(o) % 16 for o in cases["residues"]["off"][:-1]} == set(range(16))
    assert [len(cases[f"count{N}"]["which"]) for N in wc.COUNTS] == list(wc.COUNTS)
    steps = set()
    for name in ("widths", "residues", "lanes"):
        c = cases[name]
        for w, k in zip(c["windows"], c["which"]):
            steps |= ref.structure(c["structures"][k], w).steps
    assert KINDS - steps <= {"left:row0-entry"}, KINDS - steps               # the cases themselves walk through every rule as well
    for sc in wc.SCORES:                                                   # segments used, segments skipped, several copies, in both score sets
        seg = np.concatenate([wc.expected()[(n, sc)][1][0] for n in cases])
        assert (seg[:, :, 2] > 1).sum() > 100 and ((seg[:, 1, 2] == 0) & (seg[:, 0, 2] > 0)).sum() > 10 and (seg[:, 2:, 2] > 0).sum() > 10
