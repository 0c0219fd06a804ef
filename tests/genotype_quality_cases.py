"""The inputs of the genotype quality's tests, shared by the CPU tests of the reference (tests/test_genotype_quality_ref.py) and the GPU tests
(tests/test_gpu_genotype_quality.py).  A case is a dict: `case` - consensus_cases.build's numpy columns (rows, windows, support lists, allele,
zygosity) -, `qual` - the windows' qualities -, `cons_off` / `cons_bases` - the alleles' sequences, given and not voted -, and `prm` = (band_extra,
qual_cap, gap_cap, read_cap).  Everything is seeded, windows have 0..300 bases (the limit case alone is larger).  The shapes are the smallest at
which a kernel takes another path: a row of 16 lanes holds a band of up to 32 diagonals, half a wavefront one of up to 64, a wavefront one of up
to 128 with one pair of diagonals per lane and 256 with two; four tasks or two share a wavefront; a locus' entries are summed 64 at a time."""
import numpy as np

from tests import consensus_cases as cc
from tests import consensus_ref as cref
from tests import genotype_quality_ref as ref

DEFAULT = ref.DEFAULT
QUALS = (0, 1, 40, 41, 93)             # below the weights' floor, the floor, qual_cap, above it, the largest stored value


def q(w, v):
    return np.full(len(w), v, np.uint8)


def build(loci, prm, seed=0, spare_rows=3):
    """loci: per locus (zygosity, allele 0's members, allele 1's members, allele 0's sequence, allele 1's sequence); a member is (bases,
    qualities).  The span of an allele that does not exist is kept as given: it is not to be read."""
    case = cc.build([(z, [w for w, _ in a0], [w for w, _ in a1]) for z, a0, a1, _, _ in loci], prm[0], seed=seed, spare_rows=spare_rows)
    rng = np.random.default_rng(seed + 77)
    qual = rng.integers(0, 94, size=len(case["win_bases"])).astype(np.uint8)          # (the spare rows keep these)
    row_of = {(int(r), int(l)): k for k, (r, l) in enumerate(zip(case["read"], case["locus"]))}
    e = 0
    for l, (_, a0, a1, _, _) in enumerate(loci):
        for _, quals in list(a0) + list(a1):
            r = row_of[(int(case["sup_read"][e]), l)]
            qual[case["win_off"][r]:case["win_off"][r + 1]] = np.asarray(quals, np.uint8)
            e += 1
    seqs = [np.asarray(c, np.uint8) for _, _, _, c0, c1 in loci for c in (c0, c1)]
    cons_off = np.zeros(len(seqs) + 1, np.int64)
    cons_off[1:] = np.cumsum([len(c) for c in seqs])
    return dict(case=case, qual=qual, cons_off=cons_off, cons_bases=np.concatenate(seqs + [np.zeros(0, np.uint8)]).astype(np.uint8), prm=prm)


def rq(rng, w):
    """qualities drawn from QUALS"""
    return np.array(QUALS, np.uint8)[rng.integers(0, len(QUALS), size=len(w))]


BAND_DIFFS = (0, 31, 32, 63, 64, 127, 128, 255, 256)      # band_extra 0: bands of 1, 32, 33, 64, 65, 128, 129, 256 and 257 diagonals, the last unscored


def bands_case():
    """band_extra 0: per difference a locus of one allele of 40 bases whose members are longer by the difference, and one of an allele of 40 + the
    difference whose members are 40 bases: either sign.  Each has a related member and an unrelated one"""
    rng = np.random.default_rng(51)
    loci = []
    for diff in BAND_DIFFS:
        short, long_ = cc.seq(rng, 40), cc.seq(rng, 40 + diff)
        long_[:40] = short
        ws = [cc.resized(rng, long_, 40 + diff, 0.05), cc.seq(rng, 40 + diff)]
        loci.append((1, [(w, rq(rng, w)) for w in ws], [], short, cc.seq(rng, 5)))
        ws = [cc.resized(rng, short, 40, 0.05), cc.seq(rng, 40)]
        loci.append((1, [(w, rq(rng, w)) for w in ws], [], long_, cc.seq(rng, 0)))
    return build(loci, (0, 40, 20, 60), seed=1)


def wide_case():
    """band_extra 16 and 64 with zygosity 2: the two alleles of a locus fall into different buckets, and a member scoreable against allele 0
    alone (band_extra 16: 250 + 33 diagonals against allele 1) is unscored against both"""
    rng = np.random.default_rng(52)
    c0, c1 = cc.seq(rng, 40), cc.seq(rng, 130)
    c2 = np.concatenate([c0, cc.seq(rng, 250)])
    near = lambda c, n: cc.resized(rng, c, n, 0.06)      # noqa: E731
    m0 = [near(c0, 41), near(c0, 38), cc.seq(rng, 60)]
    m1 = [near(c1, 131), near(c1, 120)]
    loci = [(2, [(w, rq(rng, w)) for w in m0], [(w, rq(rng, w)) for w in m1], c0, c1),
            (2, [(w, rq(rng, w)) for w in m0[:2]], [(near(c2, 280), q(range(280), 30))], c0, c2)]
    return build(loci, DEFAULT, seed=2)


def tiny_case():
    """an empty window, an empty allele, windows of one base, against each other"""
    A, C = 0, 1
    e = np.zeros(0, np.uint8)
    one = lambda c, v: (np.array([c], np.uint8), np.array([v], np.uint8))      # noqa: E731
    loci = [(2, [(e, e), one(A, 30)], [one(C, 7), (np.array([A, C], np.uint8), np.array([50, 3], np.uint8))], np.array([A], np.uint8), e),
            (1, [(e, e), one(C, 0)], [], e, np.array([C, C], np.uint8)),
            (2, [one(A, 93)], [one(A, 1)], np.array([C, A, C], np.uint8), np.array([A, A], np.uint8))]
    return build(loci, DEFAULT, seed=3, spare_rows=0)


def gaps_case():
    """a window that lacks one base of the allele and one that has one more, at constant quality 5 (below gap_cap = 20: the gap costs 5) and 35
    (above: the gap costs 20, a substitution 35)"""
    rng = np.random.default_rng(53)
    c = np.tile(np.array([1, 0, 2, 3], np.uint8), 8)
    lacks, more = np.delete(c, 13), np.insert(c, 13, 1)
    sub = c.copy()
    sub[9] = (sub[9] + 1) % 4
    mem = [(w, q(w, v)) for v in (5, 35) for w in (lacks, more, sub)]
    return build([(1, mem, [], c, cc.seq(rng, 3))], DEFAULT, seed=4)


def flips(c0, c1, k):
    """c0 with the first k of the positions where the alleles differ taken from c1"""
    w = c0.copy()
    at = np.flatnonzero(c0 != c1)[:k]
    w[at] = c1[at]
    return w


def margins_case():
    """at constant quality 1 a window that takes k of the D positions where two equally long alleles differ scores (k, D - k).  D = 11: k = 0, 1
    and 5 give |x0 - x1| = 11, 9 and 1; D = 10: k = 0 and 5 give 10 and 0 - a tie of best, on an entry of either allele.  A locus of (5, 5)
    entries alone ties its three raw sums; one of a single (5, 6) entry ties 0/0 with 0/1; one without entries is all zeros"""
    c0 = np.tile(np.array([2, 0, 1], np.uint8), 12)
    def other(D):
        c = c0.copy()
        c[3 * np.arange(D) + 1] = 3
        return c
    c11, c10 = other(11), other(10)
    m = lambda c1, k: (flips(c0, c1, k), q(c0, 1))      # noqa: E731
    loci = [(2, [m(c11, 0), m(c11, 5)], [m(c11, 6), m(c11, 11), m(c11, 1)], c0, c11),          # (the last fits allele 0 better than its own)
            (2, [m(c10, 0), m(c10, 5)], [m(c10, 5), m(c10, 10)], c0, c10),
            (2, [m(c10, 5)], [m(c10, 5)], c0, c10),
            (2, [m(c11, 5)], [], c0, c11),
            (2, [], [], c0, c11)]
    return build(loci, DEFAULT, seed=5)


def capped_case():
    """unrelated windows at Q30: every score is far above read_cap = 60; and read_cap = 7 beside scores of 5 and 11"""
    rng = np.random.default_rng(54)
    c0, c1 = cc.seq(rng, 50), cc.seq(rng, 52)
    far = [cc.seq(rng, 50) for _ in range(3)]
    d = margins_case()
    return (build([(2, [(w, q(w, 30)) for w in far[:2]], [(far[2], q(far[2], 30))], c0, c1)], DEFAULT, seed=6),
            dict(d, prm=(16, 40, 20, 7)))


def zygosity_case():
    """zygosity 0 with and without entries, 1, 2, a locus of 70 entries (more than a wavefront's turn), and zygosity 1 with entries marked allele 1"""
    rng = np.random.default_rng(55)
    t0 = np.tile(np.array([1, 0, 2], np.uint8), 10)
    t1 = np.tile(np.array([1, 0, 2], np.uint8), 13)
    noisy = lambda t: (lambda w: (w, rq(rng, w)))(cref.noisy_read(t, 0.08, rng))      # noqa: E731
    loci = [(0, [noisy(t0), noisy(t0)], [], t0, t1), (0, [], [], t0[:0], t0[:4]), (1, [noisy(t0) for _ in range(3)], [], t0, t1),
            (2, [noisy(t0) for _ in range(35)], [noisy(t1) for _ in range(35)], t0, t1), (1, [noisy(t0), noisy(t0)], [noisy(t1)], t0, t1),
            (2, [noisy(t0)], [noisy(t1), noisy(t1)], t0, t1)]
    return build(loci, (8, 40, 20, 60), seed=7)


def rows_case(extra):
    """one-entry loci of very different lengths: the rows of a wavefront end at different steps, and the last wavefront holds 7 % 4 tasks (band_extra
    15: bands of 31 .. 33 diagonals) or 7 % 2 (band_extra 31: 63 .. 65)"""
    rng = np.random.default_rng(56 + extra)
    loci = []
    for k, n in enumerate([3, 290, 45, 260, 1, 130, 17]):
        c = cc.seq(rng, n)
        w = cc.resized(rng, c, n + k % 3, 0.05)
        loci.append((1, [(w, rq(rng, w))], [], c, c[:2]))
    return build(loci, (extra, 40, 20, 60), seed=8)


def limit_case():
    """a window above MTR_CONS_MAX_WINDOW beside one that is scored, and an allele above it: nothing of that locus is scored"""
    rng = np.random.default_rng(57)
    c = cc.seq(rng, 30)
    big = cc.seq(rng, 16385)
    w = cc.resized(rng, c, 31)
    return build([(1, [(big, q(big, 20)), (w, rq(rng, w))], [], c, c[:0]), (2, [(w, rq(rng, w))], [(c, q(c, 9))], c, big)], (2, 40, 20, 60), seed=9, spare_rows=0)


def all_cases():
    capped, cut = capped_case()
    return dict(bands=bands_case(), wide=wide_case(), tiny=tiny_case(), gaps=gaps_case(), margins=margins_case(), capped=capped, cut=cut, zygosity=zygosity_case(),
                rows=rows_case(15), halves=rows_case(31), limit=limit_case())


_cache = {}


def expected():
    """{name: (input, the reference's nine columns with the qualities, the nine without)}, computed once per process and shared by the tests; nobody
    changes it"""
    if not _cache:
        for name, d in all_cases().items():
            _cache[name] = (d, ref.genotype_quality(d["case"], d["qual"], d["cons_off"], d["cons_bases"], d["prm"]),
                            ref.genotype_quality(d["case"], None, d["cons_off"], d["cons_bases"], d["prm"]))
    return _cache


# ---- from FASTQ bytes to a genotype quality ------------------------------------------------------------------------------------------------------
# consensus_quality_cases' model and layout of reads (fq_reads: read a * FQ_READS + k is allele a's copy k).  GQ_SEED was chosen on the CPU with
# the references alone (tests/test_genotype_quality_ref.py repeats the conditions): no window has an error in its first or last two bases, the
# alleles' lengths do not meet, and BOTH the unweighted and the weighted consensus give the two true alleles.
GQ_SEED = 4      # (of seeds 0 .. 149 these hold for 4, 22, 24, 27, 111, 115 and 144; the test's own conditions for all of them but 111)


def gq_seed_is_good(seed):
    from tests import consensus_quality_cases as cqc
    from tests import consensus_quality_ref as qref

    truth = cc.truth_alleles()
    wins = cqc.fq_windows(seed)
    for a, ws in enumerate(wins):
        for w, _ in ws:
            if len(w) < 4 or w[:2].tolist() != truth[a][:2].tolist() or w[-2:].tolist() != truth[a][-2:].tolist():
                return False
    lens = [[len(w) for w, _ in ws] for ws in wins]
    if max(lens[0]) + 10 > min(lens[1]):
        return False
    case, qual = cqc.fq_case(seed)
    want = [t.tolist() for t in truth]
    seqs = lambda cons: [cons[1][cons[0][a]:cons[0][a + 1]].tolist() for a in (0, 1)]      # noqa: E731
    return seqs(cref.consensus(case, cqc.FQ_EXTRA)) == want and seqs(qref.consensus(case, qual, cqc.FQ_EXTRA, cqc.FQ_CAP)) == want


def one_side(case, side):
    """fq_case's columns with the reads of the other true allele taken out of the support lists, the calls forced to zygosity 2 over the rest"""
    from tests import consensus_quality_cases as cqc

    keep = [int(r) for r in case["sup_read"] if int(r) // cqc.FQ_READS == side]
    n = len(keep)
    return dict(case, support_off=np.array([0, n, n], np.int64), sup_read=np.array(keep, np.int32), allele=np.array([0] * ((n + 1) // 2) + [1] * (n // 2), np.uint8))


def mixed_order(case):
    """fq_case's support list with the entries either side of the alleles' border on the wrong side: the allele column that says so, and the stable
    order that makes it 0 .. 0 1 .. 1 again (the consensus requires that).  Returns (order, allele column in that order)"""
    from tests import consensus_quality_cases as cqc

    wrong = case["allele"].copy()
    wrong[cqc.FQ_READS - 1], wrong[cqc.FQ_READS] = 1, 0
    order = np.argsort(wrong, kind="stable")
    return order.astype(np.int64), wrong[order]
