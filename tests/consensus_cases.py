"""The inputs of the allele consensus' tests, shared by the CPU tests of the reference (tests/test_consensus_ref.py) and the GPU tests
(tests/test_gpu_consensus.py).  A case is a dict of numpy columns shaped as mtr_allele_consensus_device takes them - read, locus (the rows,
ascending by (read, locus)), win_off, win_bases, support_off, sup_read, allele, zygosity - with n_loci and band_extra.  Everything is seeded."""
import numpy as np

from tests import consensus_ref as ref

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33)        # either side of the 16-step direction dword, alone and summed


def seq(rng, n, alphabet=4):
    return rng.integers(0, alphabet, size=n).astype(np.uint8)


def resized(rng, truth, n, rate=0.08):
    """a noisy copy of truth brought to exactly n bases: cut, or continued with random bases"""
    w = ref.noisy_read(truth, rate, rng)
    return w[:n] if len(w) >= n else np.concatenate([w, seq(rng, n - len(w))])


def build(loci, band_extra, seed=0, spare_rows=3):
    """loci: a list of (zygosity, allele 0's windows, allele 1's windows) in list order; the entries of a locus get distinct reads drawn by the
    seed, so that a read spans several loci and the support lists are not in row order.  spare_rows rows per case support nothing."""
    rng = np.random.default_rng(seed)
    most = max([len(a0) + len(a1) for _, a0, a1 in loci] + [1])
    n_reads = most + 3
    rows = {}                                           # (read, locus) -> window
    support_off, sup_read, allele = [0], [], []
    for l, (_, a0, a1) in enumerate(loci):
        reads = rng.permutation(n_reads)[:len(a0) + len(a1)]
        for k, w in enumerate(list(a0) + list(a1)):
            rows[(int(reads[k]), l)] = np.asarray(w, np.uint8)
            sup_read.append(int(reads[k]))
            allele.append(0 if k < len(a0) else 1)
        support_off.append(len(sup_read))
    for _ in range(spare_rows):
        key = (int(rng.integers(n_reads)), int(rng.integers(len(loci))))
        rows.setdefault(key, seq(rng, int(rng.integers(0, 20))))
    keys = sorted(rows)
    win_off = np.zeros(len(keys) + 1, np.int64)
    win_off[1:] = np.cumsum([len(rows[k]) for k in keys])
    return dict(n_loci=len(loci), band_extra=band_extra, read=np.array([k[0] for k in keys], np.int32), locus=np.array([k[1] for k in keys], np.int32), win_off=win_off,
                win_bases=np.concatenate([rows[k] for k in keys] + [np.zeros(0, np.uint8)]).astype(np.uint8), support_off=np.array(support_off, np.int64),
                sup_read=np.array(sup_read, np.int32), allele=np.array(allele, np.uint8), zygosity=np.array([z for z, _, _ in loci], np.uint8))


def middle(backbone, others):
    """a member list whose backbone - position (n - 1) // 2 - is `backbone`"""
    others = list(others)
    at = len(others) // 2
    return others[:at] + [backbone] + others[at:]


def lengths_case():
    """every backbone length of LENGTHS against members of every length of LENGTHS, related and not"""
    rng = np.random.default_rng(11)
    loci = []
    for m in LENGTHS:
        truth = seq(rng, m)
        loci.append((1, middle(truth, [resized(rng, truth, n) if k % 2 == 0 else seq(rng, n) for k, n in enumerate(LENGTHS)]), []))
    return build(loci, 16, seed=1)


def bands_case():
    """band widths 63 / 64 / 65, 127 / 128 / 129, 255 / 256 / 257 (band_extra 16: length differences 30 .. 224), the member longer and shorter"""
    rng = np.random.default_rng(12)
    loci = []
    for diff in (30, 31, 32, 94, 95, 96, 222, 223, 224):
        short, long_ = seq(rng, 40), seq(rng, 40 + diff)
        long_[:40] = short
        loci.append((2, middle(short, [resized(rng, long_, 40 + diff, 0.05), resized(rng, short, 41)]), middle(long_, [resized(rng, short, 40, 0.05), resized(rng, long_, 39 + diff)])))
    return build(loci, 16, seed=2)


def members_case():
    """1, 2, 3 and 65 members per allele, low-complexity windows (ties everywhere)"""
    rng = np.random.default_rng(13)
    loci = []
    for count in (1, 2, 3, 65):
        truth = np.tile(np.array([1, 0, 2], np.uint8), 12)
        a0 = [ref.noisy_read(truth, 0.1, rng) for _ in range(count)]
        a1 = [seq(rng, int(rng.integers(20, 30)), 2) for _ in range(count)]
        loci.append((2, a0, a1))
    return build(loci, 8, seed=3)


def loci_case(n_loci):
    """63 / 64 / 65 loci, most of them empty or uncalled: zygosity 0 with and without support, zygosity 1 with entries marked allele 1 (no allele)"""
    rng = np.random.default_rng(100 + n_loci)
    loci = []
    for l in range(n_loci):
        kind = l % 8
        truth = seq(rng, 24)
        ws = [ref.noisy_read(truth, 0.1, rng) for _ in range(4)]
        if kind == 0: loci.append((2, ws[:2], ws[2:]))
        elif kind == 3: loci.append((1, ws, []))
        elif kind == 5: loci.append((0, ws[:2], []))
        elif kind == 6 and l > 40: loci.append((1, ws[:3], ws[3:]))
        else: loci.append((0, [], []))
    loci[-1] = (2, ws[:1], ws[1:])                      # the last locus is called: the lists' ends
    return build(loci, 4, seed=n_loci)


def limit_case():
    """the window limit from both sides with a small band: a backbone of 16384 bases, members of 16384 and 16380 aligned, one of 16385 skipped; and
    a backbone of 16385 bases, whose every member is skipped"""
    rng = np.random.default_rng(14)
    big = np.tile(np.array([1, 0, 2, 1, 0, 0, 3], np.uint8), 2400)[:16385]
    def near(n):
        w = big[:n].copy()
        w[rng.integers(0, n, size=40)] = 3
        return w
    return build([(2, middle(big[:16384], [near(16384), np.delete(near(16384), [5, 900, 7000, 16000]), near(16385)]), middle(big, [near(16384), near(16385)]))], 2, seed=4)


def skip_case():
    """a member skipped by the band alone (band_extra 64: 2 * 64 + 1 + 128 > 256) beside one that is not"""
    rng = np.random.default_rng(15)
    b = seq(rng, 50)
    return build([(1, middle(b, [resized(rng, b, 50 + 128), resized(rng, b, 50 + 127)]), [])], 64, seed=5)


def tiny_cases():
    """hand-sized inputs whose answers tests/test_consensus_ref.py works out by hand"""
    A, C, G, T = 0, 1, 2, 3
    return dict(
        single=build([(1, [[C, A, G]], [])], 16, spare_rows=0),
        empty_backbone=build([(1, [[A], [], [C, A]], [])], 16, spare_rows=0),
        empty_member=build([(1, [[], [C, A, G], []], [])], 16, spare_rows=0),
        uncalled=build([(0, [[C, A, G], [C, A, G]], []), (1, [[A, A], [A, A]], []), (2, [[A, C], [A, C]], [[G, G, G]])], 16, spare_rows=0))


def truth_alleles():
    cag, caa = [1, 0, 2], [1, 0, 0]
    return (np.array(cag * 10 + caa + cag * 9, np.uint8), np.array(cag * 25 + caa + cag * 6, np.uint8))     # (CAG)20 and (CAG)32, each with one CAA


TRUTH_SEEDS = (1, 2, 3)
TRUTH_READS, TRUTH_RATE, TRUTH_EXTRA = 9, 0.03, 8


def truth_windows(seed):
    """per true allele its TRUTH_READS noisy copies (3 % errors: a third each substitution, insertion, deletion)"""
    rng = np.random.default_rng(1000 + seed)
    return [[ref.noisy_read(t, TRUTH_RATE, rng) for _ in range(TRUTH_READS)] for t in truth_alleles()]


def truth_case(seed):
    """the windows as call_alleles(measure="bases") orders them: by (length, read), read = allele * TRUTH_READS + copy; the two alleles' lengths
    (60 and 96 +- a few) never meet"""
    wins = truth_windows(seed)
    rng = np.random.default_rng(seed)
    order = lambda ws, first: [w for _, _, w in sorted((len(w), first + k, w) for k, w in enumerate(ws))]      # noqa: E731
    case = build([(2, order(wins[0], 0), order(wins[1], TRUTH_READS))], TRUTH_EXTRA, seed=int(rng.integers(1 << 30)))
    return case


LETTERS = "ACGT"
TRUTH_FLANKS = ("GATTACAGGCTTCATGCAAGTCCGATAGCTTAGGCATCAG", "TTGACCGTAAGCTAGGATCCATGCAATCGGTACCTGAAGT")      # the locus: (left, "CAG", right)
OTHER_LOCUS = ("ACGGTCATTGCAAGGCTAGCTTACGGATCAGTTCAGGCAT", "GAA", "CCATGGTTAACGTCAGTCAAGGCTTACCGATGCATGCTAA")     # nothing spans it


def truth_loci():
    return [(TRUTH_FLANKS[0], "CAG", TRUTH_FLANKS[1]), OTHER_LOCUS]


def truth_reads(seed):
    """the reads of truth_windows(seed), read a * TRUTH_READS + k = allele a's copy k: 20 random bases, the left flank, the window, the right flank,
    20 random bases; every second read is the reverse complement of that (orientation 1).  The flanks are clean, so a read's window is its
    noisy repeat, base for base."""
    rng = np.random.default_rng(5000 + seed)
    code = lambda s: np.array([LETTERS.index(c) for c in s], np.uint8)      # noqa: E731
    reads = []
    for ws in truth_windows(seed):
        for w in ws:
            r = np.concatenate([seq(rng, 20), code(TRUTH_FLANKS[0]), w, code(TRUTH_FLANKS[1]), seq(rng, 20)]).astype(np.uint8)
            reads.append((3 - r[::-1]).astype(np.uint8) if len(reads) % 2 else r)
    return reads


def oriented_window(read, lo, hi, orientation):
    """what mtr_extract_windows_device defines: read[lo:hi], reverse-complemented for orientation 1"""
    w = np.asarray(read, np.uint8)[lo:hi]
    return (3 - w[::-1]).astype(np.uint8) if orientation == 1 else w.copy()


_cache = {}


def expected():
    """{name: (case, the reference's eight columns)}, computed once per process and shared by the tests; nobody changes it"""
    if not _cache:
        for name, case in all_cases().items():
            _cache[name] = (case, ref.consensus(case, case["band_extra"]))
    return _cache


def all_cases():
    cases = dict(lengths=lengths_case(), bands=bands_case(), members=members_case(), limit=limit_case(), skip=skip_case())
    for n in (63, 64, 65):
        cases[f"loci{n}"] = loci_case(n)
    cases.update(tiny_cases())
    for s in TRUTH_SEEDS:
        cases[f"truth{s}"] = truth_case(s)
    return cases
