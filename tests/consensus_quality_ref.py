"""The quality-weighted allele consensus' definition (include/mtr_hip.h, "quality-weighted allele consensus") in plain Python, written from the
header's text: the weights, the gap weights, the path column by column, the votes with their `end` counters, the emission.  D and the
directions are tests/consensus_ref.py's matrix (the alignment is not weighted); nothing of mtr_amd/csrc/banded_align.h is used.  Everything is a
list or an int; numpy appears only at the edges."""
import numpy as np

from tests import consensus_ref as ref

INS_SLOTS, MAX_CAP = ref.INS_SLOTS, 93


def weight(q, cap):
    return min(max(int(q), 1), cap)


def gap(omega, i):
    """the gap weight at boundary i (0 .. n) of a window whose base weights are omega"""
    n = len(omega)
    if n == 0:
        return 1
    if i == 0:
        return omega[0]
    if i == n:
        return omega[n - 1]
    return min(omega[i - 1], omega[i])


def columns(W, B, extra):
    """the path of W against B: per column j = 0 .. m the rows (lo_j, hi_j) and how the path leaves (lo_j, j): "diag", "left", or None for j = 0"""
    n, m = len(W), len(B)
    _, dr, _ = ref.matrix(W, B, extra)
    cols = [None] * (m + 1)
    i = n
    for j in range(m, -1, -1):
        hi = i
        while i > 0 and (j == 0 or dr[i][j] == ref.UP):
            i -= 1
        if j == 0:
            cols[0] = (i, hi, None)
        elif i > 0 and dr[i][j] == ref.DIAG:
            cols[j] = (i, hi, "diag")
            i -= 1
        else:
            cols[j] = (i, hi, "left")
    assert i == 0
    return cols


def member_votes(W, Q, B, extra, cap):
    """the votes of one aligned member: a list of ("base", j, c, w), ("del", j, w), ("ins", j, k, c, w), ("end", j, L, w)"""
    omega = [weight(q, cap) for q in Q]
    votes = []
    for j, (lo, hi, leave) in enumerate(columns(W, B, extra)):
        if leave == "diag":
            votes.append(("base", j, int(W[lo - 1]), omega[lo - 1]))
        elif leave == "left":
            votes.append(("del", j, gap(omega, lo)))
        L = hi - lo
        for k in range(min(L, INS_SLOTS)):
            votes.append(("ins", j, k, int(W[lo + k]), omega[lo + k]))
        if L < INS_SLOTS:
            votes.append(("end", j, L, gap(omega, hi)))
    return votes


def consensus_of(B, QB, members, extra, cap):
    """one allele: the backbone's window and qualities, the other members' (window, qualities).  Returns (bases, votes, aligned, skipped)"""
    m = len(B)
    omega_b = [weight(q, cap) for q in QB]
    base = [[0] * 4 for _ in range(m + 1)]
    dele = [0] * (m + 1)
    ins = [[[0] * 4 for _ in range(INS_SLOTS)] for _ in range(m + 1)]
    end = [[0] * INS_SLOTS for _ in range(m + 1)]
    for j in range(1, m + 1):
        base[j][int(B[j - 1])] += omega_b[j - 1]
    aligned = skip = 0
    for W, Q in members:
        if ref.skipped(len(W), m, extra):
            skip += 1
            continue
        aligned += 1
        for v in member_votes(W, Q, B, extra, cap):
            if v[0] == "base":
                base[v[1]][v[2]] += v[3]
            elif v[0] == "del":
                dele[v[1]] += v[2]
            elif v[0] == "ins":
                ins[v[1]][v[2]][v[3]] += v[4]
            else:
                end[v[1]][v[2]] += v[3]
    out, votes = [], []
    for j in range(m + 1):
        if j >= 1:
            top = max(base[j])
            tied = [c for c in range(4) if base[j][c] == top]
            c = int(B[j - 1]) if int(B[j - 1]) in tied else tied[0]
            if not dele[j] > top:
                out.append(c)
                votes.append(top)
        none = gap(omega_b, j)
        for k in range(INS_SLOTS):
            none += end[j][k]
            mx = max(ins[j][k])
            if not mx > none:
                break
            out.append(ins[j][k].index(mx))
            votes.append(mx)
    return out, votes, aligned, skip


def alleles(case, qual):
    """consensus_ref.alleles with every window's qualities beside it: None, or (the backbone's read, B, QB, [(W, Q), ..])"""
    both = dict(case, win_bases=np.arange(len(case["win_bases"]), dtype=np.int64))       # the same slicing gives the windows' positions
    for al in ref.alleles(both):
        if al is None:
            yield None
            continue
        rd, at, others = al
        take = lambda idx: (case["win_bases"][idx], qual[idx])      # noqa: E731
        yield (rd, *take(at), [take(o) for o in others])


def consensus(case, qual, extra, cap):
    """A whole input (tests/consensus_cases.py) with its windows' qualities -> the eight output columns as numpy, in AlleleConsensus' order"""
    assert 1 <= cap <= MAX_CAP and len(qual) == len(case["win_bases"])
    cons_off, out_b, out_v = [0], [], []
    cols = {k: [] for k in ("backbone_read", "backbone_len", "members", "aligned", "skipped")}
    for al in alleles(case, qual):
        if al is None:
            for k, v in zip(cols, (-1, 0, 0, 0, 0)):
                cols[k].append(v)
            cons_off.append(cons_off[-1])
            continue
        bb_read, B, QB, others = al
        b, v, n_al, sk = consensus_of(B, QB, others, extra, cap)
        out_b += b
        out_v += v
        cons_off.append(cons_off[-1] + len(b))
        for k, x in zip(cols, (bb_read, len(B), len(others) + 1, n_al, sk)):
            cols[k].append(x)
    return (np.array(cons_off, np.int64), np.array(out_b, np.uint8), np.array(out_v, np.int32), *[np.array(cols[k], np.int32) for k in cols])


def seeded_qualities(case, seed):
    """one Phred value 0 .. 60 per base of the case's windows"""
    return np.random.default_rng(7000 + seed).integers(0, 61, size=len(case["win_bases"])).astype(np.uint8)


def noisy_read_q(truth, rate, rng, bad=0.85):
    """consensus_ref.noisy_read's errors with qualities: a correct base draws 20 .. 39; an erroneous one (a substituted or an inserted base) 2 .. 11
    with probability `bad`, else 20 .. 39.  A deletion leaves no base and no quality.  Returns (bases, qualities)."""
    good = lambda: int(rng.integers(20, 40))                                     # noqa: E731
    wrong = lambda: int(rng.integers(2, 12)) if rng.random() < bad else good()  # noqa: E731
    out, q = [], []
    for c in truth:
        if rng.random() < rate:
            kind = int(rng.integers(3))
            if kind == 0:
                out.append((int(c) + 1 + int(rng.integers(3))) % 4)
                q.append(wrong())
            elif kind == 1:
                out += [int(rng.integers(4)), int(c)]
                q += [wrong(), good()]
        else:
            out.append(int(c))
            q.append(good())
    return np.array(out, np.uint8), np.array(q, np.uint8)


_cache = {}


def expected(name, cap):
    """(case, qualities, the reference's eight columns) of consensus_cases' case `name` at qual_cap `cap`, computed once per process"""
    from tests import consensus_cases as cc

    if "cases" not in _cache:
        _cache["cases"] = cc.all_cases()
    key = (name, cap)
    if key not in _cache:
        case = _cache["cases"][name]
        qual = seeded_qualities(case, sorted(_cache["cases"]).index(name))
        _cache[key] = (case, qual, consensus(case, qual, case["band_extra"], cap))
    return _cache[key]
