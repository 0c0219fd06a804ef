"""Inputs of the quality-weighted consensus' tests that tests/consensus_cases.py does not have: hand-sized alleles whose answers are worked out on
paper (tests/test_consensus_quality_ref.py holds the reference to them, tests/test_gpu_consensus_quality.py the GPU), and the low-depth reads
with qualities that go from FASTQ bytes to alleles."""
import numpy as np

from tests import consensus_cases as cc
from tests import consensus_quality_ref as qref

A, C, G, T = 0, 1, 2, 3


def hand_cases():
    """{name: (members in list order as (bases, qualities), qual_cap, the weighted (bases, votes), the unweighted bases)}; the backbone is the
    member at position (n - 1) // 2.  band_extra is 16 in all of them.  The paper:
    snp         CAT x3 at Q3 (one the backbone), CGT at Q30, every pair aligns diagonally.  Position 2: A = 3 + 3 + 3 = 9 against G = 30 -> G; positions
                1, 3: 9 + 30 = 39.  One vote each: A 3 against G 1 -> A.
    ins_q40     CA x3 at Q2, CGA at Q40: its G is a run of one at column 1 - ins[1][0][G] = 40, end[1][1] = min(40, 40) = 40.  The others: end[1][0] =
                min(2, 2) = 2 each, 4; the backbone's gap weight at boundary 1 is 2.  none_0 = 2 + 4 = 6 < 40: emitted with 40.  none_1 = 6 + 40 = 46 > 0:
                the junction ends.  C and A: 2 + 2 + 2 + 40 = 46.  One vote each: tot 1, N - tot = 3: not emitted.
    ins_q2      the same with the inserter at Q2: mx = 2 against none_0 = 6: not emitted; C and A: 8.
    del_q2      CT x3 at Q2 (deleters), CAT x2 at Q30 (one the backbone, position 2 of 5).  A deleter's left step at column 2 comes from row 1:
                gamma(1) = min(2, 2) = 2, del[2] = 6 against A = 30 + 30 = 60: kept.  C, T: 60 + 6 = 66.  One vote each: del 3 > A 2: deleted.
    ins_six     CA at Q30 (the backbone, position 0 of 2), C GTGTGT A at Q40: the run of six fills the four slots G T G T and casts no end vote at
                column 1; the backbone's gap weight there is 30 and no other end: 40 > 30 four times.  C, A: 30 + 40.  One vote each: 1 > 2 - 1 = 1
                is false: nothing inserted.
    empty_member   [] , CA at Q30 (backbone), []: an empty window's gap weight is 1 everywhere: del[1] = del[2] = 2 against 30: kept, votes 30.  One vote each: del 2 > 1: both deleted.
    empty_backbone A at Q40, [] (backbone), CA at Q5, Q7.  Column 0: ins[0][0] = {A: 40, C: 5}, ins[0][1] = {A: 7}, end[0][1] = 40, end[0][2] = 7; the
                empty backbone's gap weight is 1.  none_0 = 1 < 40: A with 40.  none_1 = 1 + 40 = 41 > 7: ends.  One vote each: mx 1 against N - tot = 3 -
                2 = 1: nothing."""
    q = lambda n, v: [v] * n      # noqa: E731
    return dict(
        snp=([([C, A, T], q(3, 3)), ([C, A, T], q(3, 3)), ([C, A, T], q(3, 3)), ([C, G, T], q(3, 30))], 40, ([C, G, T], [39, 30, 39]), [C, A, T]),
        ins_q40=([([C, A], q(2, 2)), ([C, A], q(2, 2)), ([C, A], q(2, 2)), ([C, G, A], q(3, 40))], 40, ([C, G, A], [46, 40, 46]), [C, A]),
        ins_q2=([([C, A], q(2, 2)), ([C, A], q(2, 2)), ([C, A], q(2, 2)), ([C, G, A], q(3, 2))], 40, ([C, A], [8, 8]), [C, A]),
        del_q2=([([C, T], q(2, 2)), ([C, T], q(2, 2)), ([C, A, T], q(3, 30)), ([C, A, T], q(3, 30)), ([C, T], q(2, 2))], 40, ([C, A, T], [66, 60, 66]), [C, T]),
        ins_six=([([C, A], q(2, 30)), ([C, G, T, G, T, G, T, A], q(8, 40))], 40, ([C, G, T, G, T, A], [70, 40, 40, 40, 40, 70]), [C, A]),
        empty_member=([([], []), ([C, A], q(2, 30)), ([], [])], 40, ([C, A], [30, 30]), []),
        empty_backbone=([([A], [40]), ([], []), ([C, A], [5, 7])], 40, ([A], [40]), []))


def hand_case_columns(members):
    """one hand case as consensus_cases' columns (one locus, zygosity 1, read k = member k, rows and entries in member order) and its qualities"""
    off = np.zeros(len(members) + 1, np.int64)
    off[1:] = np.cumsum([len(w) for w, _ in members])
    cat = lambda k, dt: np.concatenate([np.asarray(m[k], dt) for m in members] + [np.zeros(0, dt)]).astype(dt)      # noqa: E731
    n = len(members)
    case = dict(n_loci=1, band_extra=16, read=np.arange(n, dtype=np.int32), locus=np.zeros(n, np.int32), win_off=off, win_bases=cat(0, np.uint8),
                support_off=np.array([0, n], np.int64), sup_read=np.arange(n, dtype=np.int32), allele=np.zeros(n, np.uint8), zygosity=np.array([1], np.uint8))
    return case, cat(1, np.uint8)


# ---- from FASTQ bytes to alleles ------------------------------------------------------------------------------------------------------------------
# The model is made up (no basecaller was measured): consensus_ref.noisy_read's errors at FQ_RATE, an erroneous base of quality 2 .. 11 with
# probability 0.85 and 20 .. 39 otherwise, a correct base 20 .. 39 (consensus_quality_ref.noisy_read_q); the flanks and the read's ends are clean at
# Q30.  FQ_SEED was chosen on the CPU with the two references (tests/test_consensus_quality_ref.py repeats the choice's conditions): the unweighted
# consensus misses a true allele, the weighted one is both, and no read's window has an error in its first or last two bases (the flank search
# then has the window's ends where the truth has them).
FQ_SEED, FQ_READS, FQ_RATE, FQ_EXTRA, FQ_CAP = 11, 5, 0.06, 8, 40      # (of seeds 0 .. 149 the conditions hold for 11, 43 and 136)


def fq_windows(seed=FQ_SEED):
    """per true allele its FQ_READS noisy copies as (bases, qualities)"""
    rng = np.random.default_rng(9000 + seed)
    return [[qref.noisy_read_q(t, FQ_RATE, rng) for _ in range(FQ_READS)] for t in cc.truth_alleles()]


def fq_reads(seed=FQ_SEED):
    """the reads of fq_windows(seed) as consensus_cases.truth_reads lays them out - 20 random bases, the left flank, the window, the right flank, 20
    random bases, every second read reverse-complemented with its qualities reversed - as (bases, qualities) per read, read a * FQ_READS + k =
    allele a's copy k"""
    rng = np.random.default_rng(9500 + seed)
    code = lambda s: np.array([cc.LETTERS.index(c) for c in s], np.uint8)      # noqa: E731
    reads = []
    for ws in fq_windows(seed):
        for w, q in ws:
            r = np.concatenate([cc.seq(rng, 20), code(cc.TRUTH_FLANKS[0]), w, code(cc.TRUTH_FLANKS[1]), cc.seq(rng, 20)]).astype(np.uint8)
            rq = np.concatenate([np.full(60, 30, np.uint8), q, np.full(60, 30, np.uint8)]).astype(np.uint8)
            reads.append(((3 - r[::-1]).astype(np.uint8), rq[::-1].copy()) if len(reads) % 2 else (r, rq))
    return reads


def fastq_bytes(reads):
    """the reads as strict four-line FASTQ, read k named r<k>, qualities as Phred + 33"""
    out = bytearray()
    for k, (r, q) in enumerate(reads):
        out += f"@r{k}\n".encode() + bytes(cc.LETTERS[c].encode()[0] for c in r) + b"\n+\n" + bytes(int(v) + 33 for v in q) + b"\n"
    return bytes(out)


def fq_case(seed=FQ_SEED):
    """the windows of fq_windows(seed) as call_alleles(measure="bases") orders them - by (length, read) within an allele - and their qualities: one
    called locus of two (the second spans nothing), rows in read order"""
    wins = [wq for ws in fq_windows(seed) for wq in ws]
    n = len(wins)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(w) for w, _ in wins])
    order = [sorted(range(a * FQ_READS, (a + 1) * FQ_READS), key=lambda r: (len(wins[r][0]), r)) for a in (0, 1)]
    case = dict(n_loci=2, band_extra=FQ_EXTRA, read=np.arange(n, dtype=np.int32), locus=np.zeros(n, np.int32), win_off=off,
                win_bases=np.concatenate([w for w, _ in wins]).astype(np.uint8), support_off=np.array([0, n, n], np.int64),
                sup_read=np.array(order[0] + order[1], np.int32), allele=np.array([0] * FQ_READS + [1] * FQ_READS, np.uint8), zygosity=np.array([2, 0], np.uint8))
    return case, np.concatenate([q for _, q in wins]).astype(np.uint8)


def fq_seed_is_good(seed):
    """the conditions FQ_SEED was chosen by"""
    from tests import consensus_ref as ref

    truth = cc.truth_alleles()
    for a, ws in enumerate(fq_windows(seed)):
        for w, _ in ws:
            if len(w) < 4 or w[:2].tolist() != truth[a][:2].tolist() or w[-2:].tolist() != truth[a][-2:].tolist():
                return False
    lens = [[len(w) for w, _ in ws] for ws in fq_windows(seed)]
    if max(lens[0]) + 10 > min(lens[1]):
        return False
    case, qual = fq_case(seed)
    plain, weighted = ref.consensus(case, FQ_EXTRA), qref.consensus(case, qual, FQ_EXTRA, FQ_CAP)
    seqs = lambda cons: [cons[1][cons[0][a]:cons[0][a + 1]].tolist() for a in (0, 1)]      # noqa: E731
    want = [t.tolist() for t in truth]
    return seqs(weighted) == want and seqs(plain) != want
