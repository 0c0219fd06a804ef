"""The allele consensus' definition (include/mtr_hip.h, "allele consensus") in plain Python, written from the header's text and sharing no code
with mtr_amd/csrc/banded_align.h: the full (n + 1) x (m + 1) matrix with infinities outside the band, the walk, the votes, the emission, the
skip rule and the backbone choice.  Everything is a list or an int; numpy appears only at the edges."""
import numpy as np

MAX_WINDOW, MAX_BAND, INS_SLOTS = 16384, 256, 4
INF = float("inf")
DIAG, UP, LEFT = 0, 1, 2


def band(n, m, extra):
    return min(0, m - n) - extra, max(0, m - n) + extra


def skipped(n, m, extra):
    return n > MAX_WINDOW or m > MAX_WINDOW or abs(m - n) + 2 * extra + 1 > MAX_BAND


def matrix(W, B, extra, banded=True):
    """D and the directions, [n + 1][m + 1]; banded=False is the unbanded edit distance (for the tests that compare the two)"""
    n, m = len(W), len(B)
    dlo, dhi = band(n, m, extra) if banded else (-n, m)
    D = [{} for _ in range(n + 2)]                      # row i: {j: D(i, j)} for the cells that exist; a missing cell is infinite (D[-1] is empty)
    dr = [{} for _ in range(n + 1)]
    ties = set()
    for i in range(n + 1):
        for j in range(max(0, i + dlo), min(m, i + dhi) + 1):
            if i == 0 and j == 0:
                D[0][0] = 0
                continue
            diag = D[i - 1].get(j - 1, INF) + (W[i - 1] != B[j - 1]) if i >= 1 and j >= 1 else INF
            up = D[i - 1].get(j, INF) + 1 if i >= 1 else INF
            left = D[i].get(j - 1, INF) + 1 if j >= 1 else INF
            best = min(diag, up, left)
            D[i][j] = best
            dr[i][j] = DIAG if diag == best else UP if up == best else LEFT
            if diag == best and up == best:
                ties.add("diag=up")
            if up == best and left == best and diag != best:
                ties.add("up=left")
    return D, dr, ties


def walk(W, B, extra):
    """the votes of one aligned member: a list of ("base", j, c), ("del", j), ("ins", j, k, c) and the steps taken"""
    n, m = len(W), len(B)
    _, dr, _ = matrix(W, B, extra)
    votes, steps = [], []
    i, j = n, m
    while i > 0 or j > 0:
        d = dr[i][j]
        steps.append(d)
        if d == DIAG:
            votes.append(("base", j, int(W[i - 1])))
            i, j = i - 1, j - 1
        elif d == LEFT:
            votes.append(("del", j))
            j -= 1
        else:
            end = i
            i -= 1
            while i > 0 and dr[i][j] == UP:
                steps.append(UP)
                i -= 1
            for k in range(min(INS_SLOTS, end - i)):
                votes.append(("ins", j, k, int(W[i + k])))
    return votes, steps


def consensus_of(B, members, extra):
    """one allele: backbone window B, the other members' windows.  Returns (bases, votes, aligned, skipped)"""
    m = len(B)
    base = [[0] * 4 for _ in range(m + 1)]
    dele = [0] * (m + 1)
    ins = [[[0] * 4 for _ in range(INS_SLOTS)] for _ in range(m + 1)]
    for j in range(1, m + 1):
        base[j][int(B[j - 1])] += 1
    aligned = skip = 0
    for W in members:
        if skipped(len(W), m, extra):
            skip += 1
            continue
        aligned += 1
        for v in walk(W, B, extra)[0]:
            if v[0] == "base":
                base[v[1]][v[2]] += 1
            elif v[0] == "del":
                dele[v[1]] += 1
            else:
                ins[v[1]][v[2]][v[3]] += 1
    N = 1 + aligned
    out, votes = [], []
    for j in range(m + 1):
        if j >= 1:
            top = max(base[j])
            tied = [c for c in range(4) if base[j][c] == top]
            c = int(B[j - 1]) if int(B[j - 1]) in tied else tied[0]
            if not dele[j] > top:
                out.append(c)
                votes.append(top)
        for k in range(INS_SLOTS):
            tot, mx = sum(ins[j][k]), max(ins[j][k])
            if not mx > N - tot:
                break
            out.append(ins[j][k].index(mx))
            votes.append(mx)
    return out, votes, aligned, skip


def alleles(case):
    """per allele index: None without an allele, else (the backbone's read, its window B, the other members' windows in list order)"""
    read, locus, off, bases = case["read"], case["locus"], case["win_off"], case["win_bases"]
    row_of = {(int(read[r]), int(locus[r])): r for r in range(len(read))}
    win = lambda e, l: bases[int(off[row_of[(int(case["sup_read"][e]), l)]]):int(off[row_of[(int(case["sup_read"][e]), l)] + 1])]      # noqa: E731
    for A in range(2 * int(case["n_loci"])):
        l, a = divmod(A, 2)
        z = int(case["zygosity"][l])
        ents = [e for e in range(int(case["support_off"][l]), int(case["support_off"][l + 1])) if int(case["allele"][e]) == a]
        if not (z == 2 or (z == 1 and a == 0)) or not ents:
            yield None
            continue
        be = ents[(len(ents) - 1) // 2]
        yield int(case["sup_read"][be]), win(be, l), [win(e, l) for e in ents if e != be]


def consensus(case, extra):
    """A whole input (tests/consensus_cases.py: a dict of numpy columns) -> the eight output columns as numpy, in AlleleConsensus' order"""
    cons_off, out_b, out_v = [0], [], []
    cols = {k: [] for k in ("backbone_read", "backbone_len", "members", "aligned", "skipped")}
    for al in alleles(case):
        if al is None:
            for k, v in zip(cols, (-1, 0, 0, 0, 0)):
                cols[k].append(v)
            cons_off.append(cons_off[-1])
            continue
        bb_read, B, others = al
        b, v, n_al, sk = consensus_of(B, others, extra)
        out_b += b
        out_v += v
        cons_off.append(cons_off[-1] + len(b))
        for k, x in zip(cols, (bb_read, len(B), len(others) + 1, n_al, sk)):
            cols[k].append(x)
    return (np.array(cons_off, np.int64), np.array(out_b, np.uint8), np.array(out_v, np.int32), *[np.array(cols[k], np.int32) for k in cols])


def noisy_read(truth, rate, rng):
    """the seeded noise model: at every base an error with probability `rate`, a third each substitution, insertion (before the base), deletion"""
    out = []
    for c in truth:
        if rng.random() < rate:
            kind = int(rng.integers(3))
            if kind == 0:
                out.append((int(c) + 1 + int(rng.integers(3))) % 4)
            elif kind == 1:
                out += [int(rng.integers(4)), int(c)]
        else:
            out.append(int(c))
    return np.array(out, np.uint8)
