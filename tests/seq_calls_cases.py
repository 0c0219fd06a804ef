"""The inputs of the sequence allele calls' tests, shared by the CPU tests of the reference (tests/test_seq_calls_ref.py) and the GPU tests
(tests/test_gpu_seq_calls.py).  A case is (columns, prm): consensus_cases.build's dict of numpy columns - rows, windows, support lists - plus
`value`, and prm = (max_dist, min_support, min_percent, min_sep, min_gain).  Everything is seeded.  The shapes are the smallest at which a
kernel takes another path: a row of 16 lanes holds a band of up to 32 diagonals, half a wavefront one of up to 64, a wavefront one of up to 128
with one pair of diagonals per lane and 256 with two; four tasks or two share a wavefront; a locus' members are worked 64 at a time."""
import numpy as np

from tests import consensus_cases as cc
from tests import seq_calls_ref as ref

DEFAULT = (32, 2, 20, 1, 0)


def build(loci, seed=0, spare_rows=3):
    """loci: per locus the list of its members' windows in list order.  value counts up within a locus: carried along, never compared"""
    case = cc.build([(0, list(ws), []) for ws in loci], 0, seed=seed, spare_rows=spare_rows)
    case["value"] = np.concatenate([np.arange(len(ws), dtype=np.int32) * 3 + 7 + l for l, ws in enumerate(loci)] + [np.zeros(0, np.int32)]).astype(np.int32)
    del case["band_extra"], case["allele"], case["zygosity"]
    return case


def subst(rng, w, k):
    """w with exactly k positions changed (each to another base)"""
    w = np.array(w, np.uint8)
    at = rng.choice(len(w), size=k, replace=False)
    w[at] = (w[at] + rng.integers(1, 4, size=k)) % 4
    return w


def lengths_case():
    """windows of 0, 1, 2, 15, 16, 17, 31, 32, 33 bases, two of each, every pair: empty windows, length differences up to 33 against K = 20"""
    rng = np.random.default_rng(31)
    truth = cc.seq(rng, 40)
    ws = [cc.resized(rng, truth, n, 0.1) for n in cc.LENGTHS for _ in range(2)]
    return build([ws], seed=1), (20, 2, 20, 1, 0)


def limit_case():
    """two-member loci at the window limit: 16384 against 16384 and 16382 bases (computed), 16384 against 16385 and 16385 against itself (K + 1 by definition)"""
    rng = np.random.default_rng(32)
    big = cc.seq(rng, 16385)
    a = big[:16384]
    b = np.delete(subst(rng, a, 9), [700, 12000])
    return build([[a, subst(rng, a, 7)], [a, b], [a, big], [big, big.copy()]], seed=2), (32, 1, 0, 1, 0)


def zero_case():
    """K = 0: equal windows are 0, everything else 1"""
    rng = np.random.default_rng(33)
    w = cc.seq(rng, 21)
    return build([[w, w.copy(), subst(rng, w, 1), w[:20], w.copy()], [w[:1], w[:1].copy(), (w[:1] + 1) % 4], [w[:0], w[:0]]], seed=3), (0, 2, 20, 1, 0)


def exact_case():
    """K = 5: substitutions alone give a true distance of exactly K (5 changed) and K + 1 (6 changed); a tail of K bases is |length difference| = K
    (distance K), one of K + 1 bases is K + 1 by the length rule"""
    rng = np.random.default_rng(34)
    w = np.tile(np.array([1, 0, 2], np.uint8), 14)          # in a repeat a substitution cannot be bought cheaper by indels
    tail = cc.seq(rng, 6)
    return build([[w, subst(rng, w, 5), subst(rng, w, 6)], [w, np.concatenate([w, tail[:5]]), np.concatenate([w, tail])],
                  [np.concatenate([tail[:5], w]), w, np.concatenate([tail, w])]], seed=4), (5, 1, 0, 1, 0)


def bands_case(K):
    """K = 32: length differences 0 .. 5 are bands of 33, 32, 33, 32, .. diagonals, either side of the four-per-wavefront limit; K = 64: 65 and
    64, either side of two per wavefront; K = 128: 129 and 128, either side of one pair per lane; K = 254: 255 and 254.  Related windows (distance
    below K), unrelated ones (saturated), and one whose distance is exactly K by substitutions"""
    rng = np.random.default_rng(35 + K)
    n = 70 if K == 32 else 140 if K == 64 else 300
    truth = cc.seq(rng, n + 8)
    loci = []
    mono = np.zeros(n, np.uint8)                             # K of its bases changed are K edits and no fewer: nothing in it lines up better shifted
    for diff in (0, 1, 2, 3):
        a = truth[:n]
        loci.append([a, cc.resized(rng, truth, n + diff, 0.04), cc.resized(rng, truth, n - diff, 0.1), cc.seq(rng, n + diff), mono, subst(rng, mono, K), subst(rng, mono, K + 1)])
    return build(loci, seed=5), (K, 2, 20, 1, 0)


def rows_case(n_tasks, K=31):
    """n_tasks two-member loci, one task each, of very different lengths: the rows of a wavefront end at different steps, and the last wavefront
    holds n_tasks % 4 tasks.  K = 63: bands of 62 and 63 diagonals, two tasks per wavefront, the last holding n_tasks % 2"""
    rng = np.random.default_rng(40 + n_tasks + K)
    loci = []
    for k, n in enumerate([3, 900, 45, 260, 1, 130, 17][:n_tasks]):
        w = cc.seq(rng, n)
        loci.append([w, cc.resized(rng, w, n + k % 3, 0.05)])
    return build(loci, seed=6), (K, 1, 0, 1, 0)


def members_case():
    """S_l = 0, 1, 2, 3, 63, 64, 65, 128 and 129 (skipped); the members are drawn from two families of a few distinct windows each, so that costs
    tie everywhere"""
    rng = np.random.default_rng(36)
    fam = [np.tile(np.array([1, 0, 2], np.uint8), 5), np.tile(np.array([1, 0, 2, 1, 0, 0], np.uint8), 3)[:15]]
    pool = [[f, subst(rng, f, 1), subst(rng, f, 1), np.delete(f, 4)] for f in fam]
    loci = []
    for S in (0, 1, 2, 3, 63, 64, 65, 128, 129):
        loci.append([pool[int(rng.integers(2))][int(rng.integers(4))] for _ in range(S)])
    return build(loci, seed=7), (8, 2, 20, 1, 0)


def support_case():
    """S_l either side of min_support = 4: three members are no call, four are one; and 4 + 3 members, whose smaller side is below min_support"""
    rng = np.random.default_rng(37)
    a, b = cc.seq(rng, 30), cc.seq(rng, 30)
    return build([[a, a, a], [a, a, a, a], [a] * 4 + [b] * 3, [a] * 4 + [b] * 4], seed=8), (10, 4, 0, 1, 0)


def ties_case():
    """all windows identical (D = 0 everywhere: zygosity 1, the first member the medoid); two families of equal size and equal spread (cost(c)
    ties across families, cost2 ties across the medoid pairs); a family of three against one of two with min_percent 50 (not admissible)"""
    rng = np.random.default_rng(38)
    a = np.tile(np.array([1, 2, 2], np.uint8), 8)
    b = subst(rng, a, 6)
    return build([[a] * 5, [a, a, b, b], [a, b, a, b, a, b], [a, a, a, b, b]], seed=9), (32, 2, 50, 1, 0)


def sep_case(min_sep):
    """two families two substitutions apart: min_sep 2 splits them, min_sep 3 does not"""
    a = np.tile(np.array([0, 3, 1, 1], np.uint8), 6)
    b = a.copy()
    b[[5, 17]] = (b[[5, 17]] + 1) % 4
    return build([[a, a, a, b, b, b]], seed=10), (32, 2, 20, min_sep, 0)


def gain_case(min_gain):
    """three members around one centre and two three substitutions away: cost1 = 8 (the centre), the best pair's cost2 = 2, a saving of exactly
    75 % - min_gain 75 admits it, 76 does not"""
    a = np.tile(np.array([2, 0, 1], np.uint8), 8)
    b = a.copy()
    b[[3, 9, 15]] = (b[[3, 9, 15]] + 1) % 4           # three substitutions away
    c = a.copy()
    c[[4]] = (c[[4]] + 1) % 4
    d = a.copy()
    d[[10]] = (d[[10]] + 1) % 4
    return build([[a, c, d, b, b]], seed=11), (32, 2, 20, 1, min_gain)


def many_case():
    """300 small loci in one call, a third of them empty, members of two noisy families or of one"""
    rng = np.random.default_rng(39)
    loci = []
    for l in range(300):
        if l % 3 == 1:
            loci.append([])
            continue
        a = cc.seq(rng, int(rng.integers(8, 30)))
        b = subst(rng, a, min(4, len(a)))
        S = int(rng.integers(1, 9))
        loci.append([ref_noisy(rng, a if l % 2 or k % 2 else b) for k in range(S)])
    return build(loci, seed=12), (6, 2, 20, 1, 10)


def ref_noisy(rng, w):
    from tests import consensus_ref
    return consensus_ref.noisy_read(w, 0.03, rng)


def all_cases():
    cases = dict(lengths=lengths_case(), limit=limit_case(), zero=zero_case(), exact=exact_case(), members=members_case(), support=support_case(), ties=ties_case(),
                 many=many_case())
    for K in (32, 64, 128, 254):
        cases[f"bands{K}"] = bands_case(K)
    for n in (1, 2, 3, 5, 6, 7):
        cases[f"rows{n}"] = rows_case(n)
    for n in (1, 2, 3):
        cases[f"halves{n}"] = rows_case(n, 63)
    for s in (2, 3):
        cases[f"sep{s}"] = sep_case(s)
    for g in (75, 76):
        cases[f"gain{g}"] = gain_case(g)
    return cases


_cache = {}


def expected():
    """{name: (case, prm, the reference's thirteen columns)}, computed once per process and shared by the tests; nobody changes it"""
    if not _cache:
        for name, (case, prm) in all_cases().items():
            _cache[name] = (case, prm, ref.sequence_calls(case, prm))
    return _cache


# ---- from reads: two alleles of one length ------------------------------------------------------------------------------------------------------
EQUAL_SEEDS = (1, 2, 3)
EQUAL_READS, EQUAL_SUBST = 9, 2


def equal_alleles():
    cag, caa = [1, 0, 2], [1, 0, 0]
    return (np.array(cag * 20, np.uint8), np.array(cag * 10 + caa * 10, np.uint8))      # (CAG)20 and (CAG)10(CAA)10: 60 bases each, ten substitutions apart


def equal_windows(seed):
    """per true allele its EQUAL_READS copies, each with up to EQUAL_SUBST substitutions inside the repeat: every window keeps the length"""
    rng = np.random.default_rng(2000 + seed)
    return [[subst(rng, t, int(rng.integers(0, EQUAL_SUBST + 1))) for _ in range(EQUAL_READS)] for t in equal_alleles()]


def equal_reads(seed):
    """the reads of equal_windows(seed), INTERLEAVED: read 2 k + a = allele a's copy k, so that neither the read order nor the value says which
    allele a read has; built as consensus_cases.truth_reads builds its reads (clean flanks, every second read reverse-complemented)"""
    rng = np.random.default_rng(6000 + seed)
    code = lambda s: np.array([cc.LETTERS.index(c) for c in s], np.uint8)      # noqa: E731
    wins = equal_windows(seed)
    reads = []
    for k in range(EQUAL_READS):
        for a in (0, 1):
            r = np.concatenate([cc.seq(rng, 20), code(cc.TRUTH_FLANKS[0]), wins[a][k], code(cc.TRUTH_FLANKS[1]), cc.seq(rng, 20)]).astype(np.uint8)
            reads.append((3 - r[::-1]).astype(np.uint8) if len(reads) % 3 == 1 else r)
    return reads


def equal_case(seed):
    """the same windows as columns, in the list order call_alleles gives equal values: ascending read"""
    wins = equal_windows(seed)
    return build([[wins[k % 2][k // 2] for k in range(2 * EQUAL_READS)]], seed=0, spare_rows=0)
