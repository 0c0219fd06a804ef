"""The genotype quality's definition (include/mtr_hip.h, "genotype quality") in plain Python, written from the header's text and sharing no code
with mtr_amd/csrc/genotype_quality.h: the full (n + 1) x (m + 1) matrix with infinities outside tests/consensus_ref.py's band, the weights, what an
entry makes of its two scores, and the locus' sums with T written out.  tests/test_genotype_quality_ref.py holds it to an unbanded cell-by-cell
alignment and to the definition's two properties; the GPU tests (tests/test_gpu_genotype_quality.py) hold the kernels to it, column by column."""
import numpy as np

from tests import consensus_ref as cref

COLUMNS = ("score", "best", "margin", "raw", "pl", "gt", "gq", "scored", "unscored")
T = (3, 3, 2, 2, 1, 1, 1, 1, 1, 1)
INF = float("inf")
DEFAULT = (16, 40, 20, 60)             # band_extra, qual_cap, gap_cap, read_cap


def weight(q, cap):
    return min(max(int(q), 1), cap)


def gap(Q, n, i, cap):
    """gamma(i), 0 <= i <= n: the lighter of the two bases beside boundary i, the one that exists at the ends, 1 for an empty window"""
    if n == 0:
        return 1
    beside = [weight(Q[k], cap) for k in (i - 1, i) if 0 <= k < n]
    return min(beside)


def score(W, Q, C, prm, banded=True):
    """D(n, m) of window W with qualities Q (None: all qual_cap) against sequence C; banded=False is the unbanded weighted alignment"""
    extra, qual_cap, gap_cap, _ = prm
    n, m = len(W), len(C)
    Q = [qual_cap] * n if Q is None else Q
    dlo, dhi = cref.band(n, m, extra) if banded else (-n, m)
    omega = [weight(q, qual_cap) for q in Q]
    gam = [min(gap(Q, n, i, qual_cap), gap_cap) for i in range(n + 1)]
    prev = None
    for i in range(n + 1):
        cur = [INF] * (m + 1)
        for j in range(max(0, i + dlo), min(m, i + dhi) + 1):
            if i == 0 and j == 0:
                cur[0] = 0
                continue
            diag = prev[j - 1] + (omega[i - 1] if W[i - 1] != C[j - 1] else 0) if i >= 1 and j >= 1 else INF
            up = prev[j] + min(omega[i - 1], gap_cap) if i >= 1 else INF
            left = cur[j - 1] + gam[i] if j >= 1 else INF
            cur[j] = min(diag, up, left)
        prev = cur
    return int(prev[m])


def locus_columns(z, scores, read_cap):
    """raw, pl, gt, gq, scored, unscored of one locus of zygosity z from its entries' (s0, s1)"""
    if z == 0:
        return [-1] * 3, [-1] * 3, 255, -1, 0, 0
    done = [(s0, s1) for s0, s1 in scores if s0 >= 0]
    x = [(min(s0, read_cap), min(s1, read_cap)) for s0, s1 in done]
    if z == 1:
        return [sum(x0 for x0, _ in x), -1, -1], [0, -1, -1], 0, -1, len(done), len(scores) - len(done)
    h = [min(x0, x1) + 3 - (T[abs(x0 - x1)] if abs(x0 - x1) < 10 else 0) for x0, x1 in x]
    raw = [sum(x0 for x0, _ in x), sum(h), sum(x1 for _, x1 in x)]
    pl = [r - min(raw) for r in raw]
    gt = min((1, 0, 2), key=lambda g: (raw[g], (1, 0, 2).index(g)))
    return raw, pl, gt, min(pl[g] for g in range(3) if g != gt), len(done), len(scores) - len(done)


def genotype_quality(case, qual, cons_off, cons_bases, prm=DEFAULT):
    """A whole input (consensus_cases' dict of numpy columns, the windows' qualities or None, the alleles' sequences) -> the nine columns as
    numpy, in COLUMNS' order"""
    extra, read_cap = prm[0], prm[3]
    read, locus, off, bases = case["read"], case["locus"], case["win_off"], case["win_bases"]
    row_of = {(int(read[r]), int(locus[r])): r for r in range(len(read))}
    S, m = len(case["sup_read"]), int(case["n_loci"])
    sc, best, margin = np.full((S, 2), -1, np.int32), np.zeros(S, np.uint8), np.zeros(S, np.int32)
    raw, pl, gt, gq = np.zeros((m, 3), np.int64), np.zeros((m, 3), np.int64), np.zeros(m, np.uint8), np.zeros(m, np.int64)
    scored, unscored = np.zeros(m, np.int32), np.zeros(m, np.int32)
    for l in range(m):
        z = int(case["zygosity"][l])
        seqs = [cons_bases[int(cons_off[2 * l + a]):int(cons_off[2 * l + a + 1])] for a in range(z)]
        for e in range(int(case["support_off"][l]), int(case["support_off"][l + 1])):
            r = row_of[(int(case["sup_read"][e]), l)]
            W = bases[int(off[r]):int(off[r + 1])]
            Q = None if qual is None else qual[int(off[r]):int(off[r + 1])]
            best[e] = case["allele"][e]
            if z == 0 or any(cref.skipped(len(W), len(C), extra) for C in seqs):
                continue
            for a, C in enumerate(seqs):
                sc[e, a] = score(W.tolist(), None if Q is None else Q.tolist(), C.tolist(), prm)
            if z == 1:
                best[e] = 0
            elif sc[e, 0] != sc[e, 1]:
                best[e] = 0 if sc[e, 0] < sc[e, 1] else 1
            if z == 2:
                margin[e] = abs(int(sc[e, 0]) - int(sc[e, 1]))
        ents = [(int(s0), int(s1)) for s0, s1 in sc[int(case["support_off"][l]):int(case["support_off"][l + 1])]]
        raw[l], pl[l], gt[l], gq[l], scored[l], unscored[l] = locus_columns(z, ents, read_cap)
    return sc, best, margin, raw, pl, gt, gq, scored, unscored
