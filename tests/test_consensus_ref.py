"""The allele consensus' reference (tests/consensus_ref.py, the definition of include/mtr_hip.h in plain Python) held to answers worked out by
hand, and the inputs of tests/consensus_cases.py shown - from the reference alone - not to be degenerate: the GPU tests compare the library with
this reference on these inputs, so what the inputs exercise is asserted here, on the CPU."""
import numpy as np

from tests import consensus_cases as cc
from tests import consensus_ref as ref

A, C, G, T = 0, 1, 2, 3


def cons(backbone, others, extra=16):
    return ref.consensus_of(np.array(backbone, np.uint8), [np.array(w, np.uint8) for w in others], extra)


# ---- by hand --------------------------------------------------------------------------------------------------------------------------------
def test_identical_windows_walk_the_diagonal():
    votes, steps = ref.walk([C, A, G], [C, A, G], 16)
    assert steps == [ref.DIAG] * 3 and votes == [("base", 3, G), ("base", 2, A), ("base", 1, C)]


def test_diag_wins_its_tie_with_up():
    # W = AA, B = A: at (2, 1) diag = D(1, 0) + 0 = 1 and up = D(1, 1) + 1 = 1.  diag first: the spare A is an insertion BEFORE the backbone's base
    D, dr, ties = ref.matrix([A, A], [A], 16)
    assert D[2][1] == 1 and dr[2][1] == ref.DIAG and "diag=up" in ties
    assert ref.walk([A, A], [A], 16)[0] == [("base", 1, A), ("ins", 0, 0, A)]


def test_a_column_is_deleted_by_plurality_and_kept_on_a_tie():
    # W = CG against B = CAG: (2, 3) diag, (1, 2) left (1 against diag 2 and up 3), (1, 1) diag
    assert ref.walk([C, G], [C, A, G], 16)[0] == [("base", 3, G), ("del", 2), ("base", 1, C)]
    assert cons([C, A, G], [[C, G], [C, G]]) == ([C, G], [3, 3], 2, 0)                 # del 2 > base 1
    assert cons([C, A, G], [[C, G]]) == ([C, A, G], [2, 1, 2], 1, 0)                  # del 1 = base 1: the backbone's state stays


def test_an_insertion_slot_is_emitted_by_majority_only():
    assert ref.walk([C, A, G], [C, G], 16)[0] == [("base", 2, G), ("ins", 1, 0, A), ("base", 1, C)]
    assert cons([C, G], [[C, A, G], [C, A, G]]) == ([C, A, G], [3, 2, 3], 2, 0)       # 2 > 3 - 2
    assert cons([C, G], [[C, A, G]]) == ([C, G], [2, 2], 1, 0)                        # 1 > 2 - 1 fails


def test_the_fifth_base_of_an_inserted_run_votes_nothing():
    w = [C, A, A, A, A, T, G]
    votes, steps = ref.walk(w, [C, G], 16)
    assert steps.count(ref.UP) == 5
    assert votes == [("base", 2, G)] + [("ins", 1, k, A) for k in range(4)] + [("base", 1, C)]
    assert cons([C, G], [w, w]) == ([C, A, A, A, A, G], [3, 2, 2, 2, 2, 3], 2, 0)


def test_the_band_is_part_of_the_definition():
    w, b = [A, C, G, T, A, C, G, T], [C, G, T, A, C, G, T, A]                          # one shifted against the other
    assert ref.matrix(w, b, 0)[0][8][8] == 8 and ref.matrix(w, b, 0, banded=False)[0][8][8] == 2
    assert ref.matrix(w, b, 1)[0][8][8] == 2


def test_base_ties_go_to_the_backbone_else_to_the_lowest_code():
    assert cons([A], [[C]]) == ([A], [1], 1, 0)                                        # A 1, C 1: the backbone's
    assert cons([A], [[C], [C], [G], [G]]) == ([C], [2], 4, 0)                         # C 2, G 2, A 1: the lowest code


def test_one_member_is_its_own_consensus():
    case, want = cc.expected()["single"]
    assert want[0].tolist() == [0, 3, 3] and want[1].tolist() == [C, A, G] and want[2].tolist() == [1, 1, 1]
    assert want[3].tolist() == [int(case["sup_read"][0]), -1] and [w.tolist() for w in want[4:]] == [[3, 0], [1, 0], [0, 0], [0, 0]]


def test_an_empty_backbone_and_an_empty_member():
    _, want = cc.expected()["empty_backbone"]                                         # members A, (empty), CA: the slot before the first base has A 1, C 1 of N = 3
    assert want[0].tolist() == [0, 0, 0] and want[4].tolist() == [0, 0] and want[5].tolist() == [3, 0] and want[6].tolist() == [2, 0]
    _, want = cc.expected()["empty_member"]                                           # two empty members delete every column of CAG, 2 against 1
    assert want[0].tolist() == [0, 0, 0] and want[4].tolist() == [3, 0] and want[6].tolist() == [2, 0]
    assert cons([C, A, G], [[]]) == ([C, A, G], [1, 1, 1], 1, 0)                      # one of them ties: kept


def test_zygosity_0_1_and_2():
    case, want = cc.expected()["uncalled"]
    assert case["zygosity"].tolist() == [0, 1, 2]
    assert want[0].tolist() == [0, 0, 0, 2, 2, 4, 7]
    assert want[1].tolist() == [A, A, A, C, G, G, G] and want[2].tolist() == [2, 2, 2, 2, 1, 1, 1]
    assert want[3].tolist()[:2] == [-1, -1] and want[3].tolist()[3] == -1 and want[5].tolist() == [0, 0, 2, 0, 2, 1]


def test_orientation_1_reads_in_the_locus_direction():
    read = [A, C, G, T, T]
    assert cc.oriented_window(read, 1, 4, 0).tolist() == [C, G, T] and cc.oriented_window(read, 1, 4, 1).tolist() == [A, C, G]
    assert cc.oriented_window(read, 2, 2, 1).tolist() == []


# ---- the cases are not degenerate ------------------------------------------------------------------------------------------------------------
def pairs(case):
    for al in ref.alleles(case):
        if al is not None:
            for w in al[2]:
                if not ref.skipped(len(w), len(al[1]), case["band_extra"]):
                    yield w, al[1]


def test_every_direction_and_both_ties_occur():
    steps, ties = set(), set()
    for name in ("lengths", "members"):
        case = cc.expected()[name][0]
        for w, b in pairs(case):
            steps |= set(ref.walk(w, b, case["band_extra"])[1])
            ties |= ref.matrix(w, b, case["band_extra"])[2]
    assert steps == {ref.DIAG, ref.UP, ref.LEFT} and ties == {"diag=up", "up=left"}


def test_the_shapes_the_kernel_can_go_wrong_at():
    ex = cc.expected()
    case = ex["lengths"][0]
    seen = {(len(w), len(b)) for w, b in pairs(case)}
    assert {n for n, _ in seen} == set(cc.LENGTHS) and {m for _, m in seen} == set(cc.LENGTHS)
    assert {(n + m) % 16 for n, m in seen} >= {15, 0, 1}
    case, want = ex["bands"]
    widths = set()
    for al in ref.alleles(case):
        for w in al[2]:
            widths.add(abs(len(al[1]) - len(w)) + 2 * case["band_extra"] + 1)
    assert widths >= {63, 64, 65, 127, 128, 129, 255, 256, 257}
    assert sum(want[7].tolist()) == 2 and all(s == 0 or a == 1 for s, a in zip(want[7].tolist(), want[6].tolist()))      # 257 is skipped, as the longer and as the shorter
    assert ex["members"][1][5].tolist() == [1, 1, 2, 2, 3, 3, 65, 65]
    for n in (63, 64, 65):
        case, want = ex[f"loci{n}"]
        assert case["n_loci"] == n and (want[3] < 0).sum() > n and want[3][-1] >= 0 and want[3][-2] >= 0
        z1 = [l for l in range(n) if case["zygosity"][l] == 1 and (case["allele"][case["support_off"][l]:case["support_off"][l + 1]] == 1).any()]
        assert z1 and all(want[3][2 * l + 1] == -1 for l in z1)                         # entries marked allele 1 at zygosity 1 are no allele


def test_each_skip_condition_alone():
    case, want = cc.expected()["limit"]
    assert want[4].tolist() == [16384, 16385] and want[5].tolist() == [4, 3] and want[6].tolist() == [2, 0] and want[7].tolist() == [1, 2]
    assert ref.skipped(16385, 16384, 2) and not ref.skipped(16384, 16384, 2) and not ref.skipped(16380, 16384, 2)       # n alone
    assert ref.skipped(16384, 16385, 2)                                                                                # m alone
    assert (want[0][1], want[0][2] - want[0][1]) == (len(want[1]) - 16385, 16385)                                      # no member aligned: the backbone itself
    case, want = cc.expected()["skip"]
    assert want[6].tolist()[0] == 1 and want[7].tolist()[0] == 1                                                       # 2 * 64 + 1 + 128 = 257 > 256 >= 2 * 64 + 1 + 127


def test_votes_never_exceed_the_voters():
    for name, (case, want) in cc.expected().items():
        per = np.repeat(1 + want[6], np.diff(want[0]))
        assert (want[2] >= 1).all() and (want[2] <= per).all(), name


# ---- consensus finds the truth ---------------------------------------------------------------------------------------------------------------
def test_the_consensus_is_the_true_allele_on_the_seeds_the_gpu_test_uses():
    """9 reads per allele at 3 % errors (a third each substitution, insertion, deletion), band_extra 8: the reference's consensus of both alleles is
    the truth, the CAA interruption included, on every seed of TRUTH_SEEDS.  (Chosen seeds: the reference decides, and it is asserted here.)"""
    truth = cc.truth_alleles()
    assert len(truth[0]) == 60 and len(truth[1]) == 96 and truth[0][30:33].tolist() == [C, A, A] and truth[1][75:78].tolist() == [C, A, A]
    for seed in cc.TRUTH_SEEDS:
        case, want = cc.expected()[f"truth{seed}"]
        assert want[5].tolist() == [cc.TRUTH_READS] * 2 and want[7].tolist() == [0, 0]
        wins = cc.truth_windows(seed)
        assert any(len(w) != len(t) or (w != t).any() for ws, t in zip(wins, truth) for w in ws)                      # the reads are noisy
        for a in (0, 1):
            assert want[1][want[0][a]:want[0][a + 1]].tolist() == truth[a].tolist(), (seed, a)
