"""The sequence allele calls' reference (tests/seq_calls_ref.py) on the CPU: held to a brute force that shares nothing with it - a cell-by-cell
Levenshtein and a split written as loops over members - on a few hundred seeded loci of at most 8 members, to hand-worked answers, and shown
to meet, on the cases of tests/seq_calls_cases.py, the situations those cases are there for.  The last test states what the feature is for: two
alleles of one length are one allele to the calls by value, two to the calls by sequence, and the consensus over the latter is the truth.
The library must offer the entry points: without them nothing here has a subject."""
import itertools

import numpy as np
import pytest

import mtr_amd
from tests import allele_call_ref
from tests import consensus_cases as cc
from tests import consensus_ref
from tests import seq_calls_cases as sc
from tests import seq_calls_ref as ref


@pytest.fixture(scope="module", autouse=True)
def the_entry_points_exist():
    lib = mtr_amd.load_library()
    assert hasattr(lib, "mtr_call_alleles_sequence_device") and hasattr(lib, "mtr_call_alleles_sequence_copy_device")


def brute_lev(a, b):
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D[len(a)][len(b)]


def test_the_distance_is_levenshtein_saturated():
    rng = np.random.default_rng(1)
    assert ref.lev([], []) == 0 and ref.lev([1], []) == 1 and ref.lev([], [0, 1]) == 2
    assert ref.lev([1, 0, 2, 1, 0, 2], [1, 0, 0, 1, 0, 2]) == 1 and ref.lev([0, 1, 2, 3], [1, 2, 3, 0]) == 2          # kitten-sized, by hand
    for _ in range(300):
        a, b = cc.seq(rng, int(rng.integers(0, 14)), 3), cc.seq(rng, int(rng.integers(0, 14)), 3)
        want = brute_lev(a.tolist(), b.tolist())
        assert ref.lev(a, b) == want == ref.lev(b, a)
        for K in (0, 1, 3, 20):
            assert ref.distance(a, b, K) == (K + 1 if abs(len(a) - len(b)) > K else min(want, K + 1))
    big = np.zeros(ref.MAX_WINDOW + 1, np.uint8)
    assert ref.distance(big, big, 7) == 8 and ref.distance(big[:-1], big[:-1], 7) == 0


def test_the_pair_index_walks_the_upper_triangle_row_by_row():
    for S in (2, 3, 7, 128):
        assert [ref.pair_index(S, t, u) for t in range(S) for u in range(t + 1, S)] == list(range(S * (S - 1) // 2))


def _small_case(seed):
    rng = np.random.default_rng(seed)
    loci = []
    for _ in range(25):
        a = cc.seq(rng, int(rng.integers(3, 12)), 3)
        b = sc.subst(rng, a, int(rng.integers(1, 4)))
        loci.append([consensus_ref.noisy_read(a if rng.integers(2) else b, 0.08, rng) for _ in range(int(rng.integers(0, 9)))])
    prm = (int(rng.integers(0, 6)), int(rng.integers(1, 4)), int(rng.integers(0, 51)), int(rng.integers(1, 4)), int(rng.integers(0, 60)))
    return sc.build(loci, seed=seed), prm


@pytest.mark.parametrize("seed", range(12))
def test_the_invariants_on_small_loci_against_brute_force(seed):
    """12 x 25 loci of 0 .. 8 members"""
    case, prm = _small_case(seed)
    K, min_support, min_percent, min_sep, min_gain = prm
    got = dict(zip(ref.COLUMNS, ref.sequence_calls(case, prm)))
    for l, wins in enumerate(ref.members(case)):
        S, lo, po = len(wins), int(case["support_off"][l]), int(got["pair_off"][l])
        full = [[brute_lev(a.tolist(), b.tolist()) for b in wins] for a in wins]
        D = [[min(full[t][u], K + 1) for u in range(S)] for t in range(S)]
        for t, u in itertools.combinations(range(S), 2):
            d = int(got["dist"][po + ref.pair_index(S, t, u)])
            assert d == D[t][u] and (d == K + 1 or d == full[t][u])             # every distance that is not K + 1 is the unbanded distance
        assert int(got["pair_off"][l + 1]) - po == S * (S - 1) // 2
        allele, z = got["allele"][lo:lo + S].tolist(), int(got["zygosity"][l])
        assert allele == sorted(allele) and (z == 2) == (1 in allele)             # 0 .. 0 1 .. 1
        reads = got["read"][lo:lo + S].tolist()
        place = {int(r): k for k, r in enumerate(case["sup_read"][lo:lo + S])}
        assert sorted(reads) == sorted(place) and got["value"][lo:lo + S].tolist() == [int(case["value"][lo + place[r]]) for r in reads]
        for al in (0, 1):
            mine = [place[r] for r, x in zip(reads, allele) if x == al]
            assert mine == sorted(mine)                                           # the partition is stable
        if S < min_support:
            assert z == 0 and got["medoid"][l].tolist() == [-1, -1] and not got["cost"][l].any() and not got["call_support"][l].any()
            continue
        costs = [sum(D[c]) for c in range(S)]
        cost1 = min(costs)
        options = []                                                              # every admissible pair, by brute force
        for c0, c1 in itertools.combinations(range(S), 2):
            side = [0 if D[c0][u] <= D[c1][u] else 1 for u in range(S)]
            n0, n1 = side.count(0), side.count(1)
            cost2 = sum(min(D[c0][u], D[c1][u]) for u in range(S))
            if min(n0, n1) >= min_support and min(n0, n1) * 100 >= min_percent * S and D[c0][c1] >= min_sep and cost2 * 100 <= cost1 * (100 - min_gain):
                options.append((cost2, c0, c1, side))
        if not options:
            assert z == 1 and got["cost"][l].tolist() == [cost1, cost1] and got["call_support"][l].tolist() == [S, 0]
            assert place[int(got["medoid"][l, 0])] == costs.index(cost1) and got["medoid"][l, 1] == -1
            assert got["dist_to_medoid"][lo:lo + S].tolist() == D[costs.index(cost1)] and reads == case["sup_read"][lo:lo + S].tolist()
            continue
        cost2, c0, c1, side = min(options)
        assert z == 2 and got["cost"][l].tolist() == [cost1, cost2] and cost2 == min(o[0] for o in options)          # a least-cost admissible pair
        assert [place[int(r)] for r in got["medoid"][l]] == [c0, c1] and got["call_support"][l].tolist() == [side.count(0), side.count(1)]
        assert [side[place[r]] for r in reads] == allele
        assert got["dist_to_medoid"][lo:lo + S].tolist() == [D[(c0, c1)[side[place[r]]]][place[r]] for r in reads]
        assert got["call"][l].tolist() == [int(case["value"][lo + c0]), int(case["value"][lo + c1])]


def _col(name, which):
    case, prm, want = sc.expected()[name]
    return dict(zip(ref.COLUMNS, want))[which]


def test_the_cases_meet_what_they_are_there_for():
    assert _col("zero", "dist").tolist() == [0, 1, 1, 0, 1, 1, 0, 1, 1, 1] + [0, 1, 1] + [0]
    # exactly K, K + 1 by value, K + 1 by value; a tail of K bases, of K + 1 (the length rule), the two tails one base apart; the same with heads
    assert _col("exact", "dist").tolist() == [5, 6, 6, 5, 6, 1, 5, 1, 6]
    assert _col("limit", "dist").tolist() == [7, 11, 33, 33] and _col("limit", "zygosity").tolist() == [2, 2, 2, 2]      # (min_support 1)
    assert _col("members", "skipped").tolist() == [0] * 8 + [1] and _col("members", "zygosity").tolist()[-1] == 0
    assert np.diff(_col("members", "pair_off")).tolist() == [0, 0, 1, 3, 1953, 2016, 2080, 8128, 0]
    assert set(_col("members", "zygosity").tolist()[4:8]) == {2}
    assert _col("support", "zygosity").tolist() == [0, 1, 1, 2]
    assert _col("ties", "zygosity").tolist() == [1, 2, 2, 1] and not _col("ties", "dist")[:10].any() and _col("ties", "medoid")[0, 1] == -1
    assert _col("sep2", "zygosity").tolist() == [2] and _col("sep3", "zygosity").tolist() == [1] and set(_col("sep2", "dist").tolist()) == {0, 2}
    assert _col("gain75", "zygosity").tolist() == [2] and _col("gain76", "zygosity").tolist() == [1] and _col("gain75", "cost").tolist() == [[8, 2]]
    lengths = _col("lengths", "dist")
    assert 0 < (lengths == 21).sum() < len(lengths) and (lengths < 21).sum() > 40
    for K in (32, 64, 128, 254):
        d = _col(f"bands{K}", "dist")
        assert (d == K).any() and (d == K + 1).any() and (d < K).sum() >= 8, K
    z = _col("many", "zygosity")
    assert (z == 0).sum() > 100 and (z == 1).sum() > 20 and (z == 2).sum() > 20


def test_the_band_widths_the_cases_name():
    def widths(name):
        case, prm, _ = sc.expected()[name]
        out = set()
        for wins in ref.members(case):
            for a, b in itertools.combinations(wins, 2):
                diff = abs(len(a) - len(b))
                if diff <= prm[0] and len(a) and len(b):
                    out.add(diff + 2 * ((prm[0] - diff) >> 1) + 1)
        return out
    assert {32, 33} <= widths("bands32") and {64, 65} <= widths("bands64") and {128, 129} <= widths("bands128") and {254, 255} <= widths("bands254")
    assert all(max(widths(f"rows{n}")) <= 32 for n in (1, 2, 3, 5, 6, 7)) and all(widths(f"halves{n}") <= {62, 63, 64} for n in (1, 2, 3))


@pytest.mark.parametrize("seed", sc.EQUAL_SEEDS)
def test_two_alleles_of_one_length_are_told_apart_by_sequence_alone(seed):
    case = sc.equal_case(seed)
    truth = sc.equal_alleles()
    n = 2 * sc.EQUAL_READS
    assert all(len(w) == 60 for w in ref.members(case)[0])
    assert allele_call_ref.split([60] * n, 2, 20, 1)[0] == 1                          # by value: one allele
    got = dict(zip(ref.COLUMNS, ref.sequence_calls(case, sc.DEFAULT)))
    assert got["zygosity"].tolist() == [2] and got["call_support"].tolist() == [[sc.EQUAL_READS] * 2]
    place = {int(r): k for k, r in enumerate(case["sup_read"])}                       # list position k holds allele k % 2's copy k // 2
    sides = [place[int(r)] % 2 for r in got["read"]]
    assert sides == [sides[0]] * sc.EQUAL_READS + [1 - sides[0]] * sc.EQUAL_READS     # partitioned by the true allele; which one is called first is the medoids' order
    called = dict(case, band_extra=8, sup_read=got["read"], allele=got["allele"], zygosity=got["zygosity"])
    cons = consensus_ref.consensus(called, 8)
    for a in (0, 1):
        assert cons[1][cons[0][a]:cons[0][a + 1]].tolist() == truth[a ^ sides[0]].tolist(), (seed, a)
