"""tests/genotype_quality_ref.py, the genotype quality's definition in plain Python, held to things that share nothing with it (CPU): an unbanded
weighted alignment computed by recursion over prefixes wherever the band cannot bind, the definition's two properties against the consensus'
reference matrix, T against its formula; and the inputs of tests/genotype_quality_cases.py shown to meet the situations they are there for -
by the reference's own columns, since the GPU test compares nothing else."""
import functools
import math
import sys

import numpy as np
import pytest

from tests import consensus_cases as cc
from tests import consensus_quality_cases as cqc
from tests import consensus_ref as cref
from tests import genotype_quality_cases as gc
from tests import genotype_quality_ref as ref


def unbanded(W, Q, C, qual_cap, gap_cap):
    """the cheapest weighted alignment of W[:i] with C[:j], by recursion; no band"""
    n = len(W)
    w = lambda k: min(max(Q[k], 1), qual_cap)      # noqa: E731

    def gamma(i):
        if n == 0:
            return 1
        return w(0) if i == 0 else w(n - 1) if i == n else min(w(i - 1), w(i))

    @functools.lru_cache(maxsize=None)
    def go(i, j):
        if i == 0 and j == 0:
            return 0
        ways = []
        if i and j:
            ways.append(go(i - 1, j - 1) + (w(i - 1) if W[i - 1] != C[j - 1] else 0))
        if i:
            ways.append(go(i - 1, j) + min(w(i - 1), gap_cap))
        if j:
            ways.append(go(i, j - 1) + min(gamma(i), gap_cap))
        return min(ways)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(10000)
    try:
        return go(n, len(C))
    finally:
        sys.setrecursionlimit(limit)


def test_the_score_is_the_unbanded_weighted_alignment_where_the_band_cannot_bind():
    rng = np.random.default_rng(5)
    for k in range(300):
        n, m = int(rng.integers(0, 25)), int(rng.integers(0, 25))
        W = cc.seq(rng, n, 2 + k % 3).tolist()
        C = (cc.resized(rng, np.array(W, np.uint8), m, 0.2) if k % 2 and n else cc.seq(rng, m)).tolist()
        Q = rng.integers(0, 94, size=n).tolist() if k % 3 else np.array(gc.QUALS)[rng.integers(0, 5, size=n)].tolist()
        qual_cap = int(rng.integers(1, 94))
        gap_cap = int(rng.integers(1, qual_cap + 1))
        extra = max(n, m) + int(rng.integers(0, 3))
        assert ref.score(W, Q, C, (extra, qual_cap, gap_cap, 60)) == unbanded(W, Q, C, qual_cap, gap_cap), (k, W, Q, C, qual_cap, gap_cap)
        assert ref.score(W, None, C, (extra, qual_cap, gap_cap, 60)) == unbanded(W, [qual_cap] * n, C, qual_cap, gap_cap), k


def test_weights_of_one_give_the_unit_distance_and_a_constant_quality_its_multiple():
    rng = np.random.default_rng(6)
    for k in range(200):
        n, m, extra = int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(0, 10))
        W, C = cc.seq(rng, n).tolist(), cc.seq(rng, m).tolist()
        if k % 2 and n:
            C = cc.resized(rng, np.array(W, np.uint8), m, 0.1).tolist()
        Q = rng.integers(0, 94, size=n).tolist()
        unit = cref.matrix(W, C, extra)[0][n][m]                # the consensus' banded D(n, m)
        assert ref.score(W, Q, C, (extra, 1, 1, 60)) == unit, k
        if n:
            gap_cap = int(rng.integers(1, 41))
            c = int(rng.integers(1, gap_cap + 1))
            assert ref.score(W, [c] * n, C, (extra, 40, gap_cap, 60)) == c * unit, k


def test_the_table_is_its_formula_rounded():
    assert [round(10 * math.log10(1 + 10 ** (-d / 10))) for d in range(10)] == list(ref.T)
    assert all(10 * math.log10(1 + 10 ** (-d / 10)) < 0.5 for d in range(10, 200))


# ---- the cases meet their situations ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exp():
    return gc.expected()


def _entries(d):
    """per support entry (locus, zygosity, n, [m of the existing alleles])"""
    case = d["case"]
    row_of = {(int(r), int(l)): k for k, (r, l) in enumerate(zip(case["read"], case["locus"]))}
    out = []
    for l in range(case["n_loci"]):
        z = int(case["zygosity"][l])
        ms = [int(d["cons_off"][2 * l + a + 1] - d["cons_off"][2 * l + a]) for a in range(z)]
        for e in range(int(case["support_off"][l]), int(case["support_off"][l + 1])):
            r = row_of[(int(case["sup_read"][e]), l)]
            out.append((l, z, int(case["win_off"][r + 1] - case["win_off"][r]), ms))
    return out


def _widths(d):
    return sorted({abs(m - n) + 2 * d["prm"][0] + 1 for _, _, n, ms in _entries(d) for m in ms})


def test_the_bands_lie_on_both_sides_of_every_bucket_border_with_either_sign(exp):
    d, want, _ = exp["bands"]
    assert _widths(d) == [1, 32, 33, 64, 65, 128, 129, 256, 257]
    signs = {(abs(m - n) + 1, (m > n) - (m < n)) for _, _, n, ms in _entries(d) for m in ms}
    assert all((w, s) in signs for w in (32, 33, 64, 65, 128, 129, 256, 257) for s in (-1, 1))
    unscored = [k for k, (_, _, n, ms) in enumerate(_entries(d)) if abs(ms[0] - n) == 256]
    assert len(unscored) == 4 and all(want[0][k].tolist() == [-1, -1] for k in unscored)
    assert all(want[0][k][0] >= 0 for k in range(len(want[0])) if k not in unscored) and want[8].sum() == 4
    assert [w for w in _widths(exp["rows"][0]) if w <= 33] == [31, 32, 33] and _widths(exp["halves"][0]) == [63, 64, 65]
    assert max(n for _, _, n, _ in _entries(d)) <= 300


def test_empty_and_one_base_sequences_and_every_special_quality(exp):
    d, want, _ = exp["tiny"]
    ent = _entries(d)
    assert any(n == 0 for _, _, n, _ in ent) and any(0 in ms for _, _, _, ms in ent) and any(n == 1 for _, _, n, _ in ent) and any(n == 0 and 0 in ms for _, _, n, ms in ent)
    assert (want[0][[k for k, (_, z, _, _) in enumerate(ent) if z == 2]] >= 0).all()
    for name in ("bands", "wide", "zygosity"):
        assert set(gc.QUALS) <= set(exp[name][0]["qual"].tolist()), name
    assert gc.QUALS == (0, 1, 40, 41, 93) and all(exp[name][0]["prm"][1] == 40 for name in ("bands", "wide", "zygosity"))
    assert any(not np.array_equal(exp[name][1][0], exp[name][2][0]) for name in exp)          # the qualities matter


def test_the_gap_cap_binds_above_the_qualities_and_not_below(exp):
    d, want, _ = exp["gaps"]
    assert want[0][:, 0].tolist() == [5, 5, 5, 20, 20, 35] and d["prm"][2] == 20           # Q5: the gap costs 5 as a substitution does; Q35: the gap 20, the substitution 35
    loose = ref.genotype_quality(d["case"], d["qual"], d["cons_off"], d["cons_bases"], (16, 40, 40, 60))
    assert loose[0][:, 0].tolist() == [5, 5, 5, 35, 35, 35]


def test_the_margins_the_ties_and_the_caps(exp):
    d, want, _ = exp["margins"]
    col = dict(zip(ref.COLUMNS, want))
    assert sorted(set(col["margin"].tolist())) == [0, 1, 9, 10, 11]
    ties = [k for k in range(len(col["margin"])) if col["score"][k, 0] == col["score"][k, 1]]
    assert {int(d["case"]["allele"][k]) for k in ties} == {0, 1} and all(col["best"][k] == d["case"]["allele"][k] for k in ties)
    assert any(col["best"][k] != d["case"]["allele"][k] for k in range(len(col["best"])))      # and a read that fits the other allele better
    assert col["raw"][2].tolist() == [10, 10, 10] and col["gt"][2] == 1 and col["gq"][2] == 0       # a three-way tie: 0/1
    assert col["raw"][3].tolist() == [5, 5, 6] and col["gt"][3] == 1 and col["gq"][3] == 0          # 0/0 ties with 0/1: 0/1
    assert col["raw"][4].tolist() == [0, 0, 0] and col["scored"][4] == 0 and d["case"]["support_off"][4] == d["case"]["support_off"][5]      # no entries
    cut = dict(zip(ref.COLUMNS, exp["cut"][1]))
    assert exp["cut"][0]["prm"][3] == 7 and np.array_equal(cut["score"], col["score"]) and not np.array_equal(cut["raw"], col["raw"])
    assert col["score"][:5].tolist() == [[0, 11], [5, 6], [6, 5], [11, 0], [1, 10]] and cut["raw"][0].tolist() == [19, 17, 25]      # by hand: (0, 7) (5, 6) (6, 5) (7, 0) (1, 7)
    far = dict(zip(ref.COLUMNS, exp["capped"][1]))
    assert (far["score"] > 60).all() and far["raw"][0].tolist() == [180, 180, 180]


def test_the_zygosities_the_long_locus_and_the_unscored_entries(exp):
    d, want, _ = exp["zygosity"]
    col = dict(zip(ref.COLUMNS, want))
    off = d["case"]["support_off"]
    assert d["case"]["zygosity"].tolist() == [0, 0, 1, 2, 1, 2] and (off[1:] - off[:-1]).tolist() == [2, 0, 3, 70, 3, 3]
    assert col["gt"].tolist()[:3] == [255, 255, 0] and col["raw"][0].tolist() == [-1, -1, -1] and col["pl"][2].tolist() == [0, -1, -1] and col["gq"].tolist()[:3] == [-1, -1, -1]
    assert (col["score"][:2] == -1).all() and col["scored"].tolist() == [0, 0, 3, 70, 3, 3] and (col["score"][2:5, 1] == -1).all()
    assert col["gt"][3] == 1 and col["gq"][3] > 0
    assert d["case"]["allele"][off[4]:off[5]].tolist() == [0, 0, 1] and col["best"][off[4]:off[5]].tolist() == [0, 0, 0]
    w, wide, _ = exp["wide"]
    assert wide[7].tolist() == [5, 0] and wide[8].tolist() == [0, 3] and (wide[0][5:] == -1).all()       # locus 1: its third member is too far from allele 1, its first two from it too
    ent = _entries(w)
    assert [cref.skipped(ent[7][2], m, 16) for m in ent[7][3]] == [True, False] and [cref.skipped(ent[5][2], m, 16) for m in ent[5][3]] == [False, True]
    lim, big, _ = exp["limit"]
    ent = _entries(lim)
    assert ent[0][2] == 16385 and ent[2][3][1] == 16385 and big[0].tolist() == [[-1, -1], [big[0][1, 0], -1], [-1, -1], [-1, -1]] and big[0][1, 0] >= 0
    assert big[8].tolist() == [1, 2]


# ---- from FASTQ bytes ------------------------------------------------------------------------------------------------------------------------------
def test_the_chosen_seed_meets_the_conditions_of_the_gpu_test_under_the_references():
    seed = gc.GQ_SEED
    assert gc.gq_seed_is_good(seed)
    case, qual = cqc.fq_case(seed)
    prm = (cqc.FQ_EXTRA, 40, 20, 60)
    cons = cref.consensus(case, cqc.FQ_EXTRA)
    col = dict(zip(ref.COLUMNS, ref.genotype_quality(case, qual, cons[0], cons[1], prm)))
    assert col["gt"].tolist() == [1, 255] and col["gq"][0] > 0
    assert col["best"].tolist() == [int(r) // cqc.FQ_READS for r in case["sup_read"]]
    for side in (0, 1):
        hom = dict(zip(ref.COLUMNS, ref.genotype_quality(gc.one_side(case, side), qual, cons[0], cons[1], prm)))
        assert hom["gt"][0] == 2 * side and hom["gq"][0] > 0, side
    # two reads put on the wrong side by hand: the consensus over those calls misses the truth, every read's best is still its true side, and the
    # consensus over the reassigned calls is the truth again
    import mtr_amd
    torch = pytest.importorskip("torch")
    truth = [t.tolist() for t in cc.truth_alleles()]
    seqs = lambda c: [c[1][c[0][a]:c[0][a + 1]].tolist() for a in (0, 1)]      # noqa: E731
    order, wrong = gc.mixed_order(case)
    mixed = dict(case, sup_read=case["sup_read"][order], allele=wrong)
    assert seqs(cref.consensus(mixed, cqc.FQ_EXTRA)) != truth
    got = ref.genotype_quality(mixed, qual, cons[0], cons[1], prm)
    assert got[1].tolist() == [int(r) // cqc.FQ_READS for r in mixed["sup_read"]] and got[1].tolist() != wrong.tolist()
    t = torch.from_numpy
    calls = mtr_amd.AlleleCalls(t(mixed["support_off"]), torch.zeros(len(wrong), dtype=torch.int32), t(mixed["sup_read"]), t(wrong), t(case["zygosity"]),
                                torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64))
    fixed = mtr_amd.with_reassigned_alleles(calls, mtr_amd.GenotypeQuality(*[t(np.ascontiguousarray(c)) for c in got]))
    assert seqs(cref.consensus(dict(mixed, sup_read=fixed.read.numpy(), allele=fixed.allele.numpy()), cqc.FQ_EXTRA)) == truth
