"""The sequence allele calls in plain Python / numpy, worded as include/mtr_hip.h ("sequence allele calls") words them: a full-matrix Levenshtein
distance (row by row, nothing banded), its saturation at K + 1 with the two rules that make a pair K + 1 by definition, the one- and two-medoid
enumeration over every pair c0 < c1, and the stable partition.  tests/test_seq_calls_ref.py holds it to a brute force that shares nothing with
it; the GPU tests (tests/test_gpu_seq_calls.py) hold the kernels to it, column by column."""
import numpy as np

MAX_WINDOW, MAX_DIST, MAX_MEMBERS = 16384, 254, 128
COLUMNS = ("support_off", "value", "read", "allele", "zygosity", "call", "call_support", "cost", "medoid", "dist_to_medoid", "skipped", "pair_off", "dist")


def lev(a, b):
    """the unit-cost edit distance, the whole matrix, one row at a time; the row's run of `left` steps is a running minimum of D[j] - j"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    m = len(b)
    idx = np.arange(m + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(1, len(a) + 1):
        cur = np.empty(m + 1, np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (b != a[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(cur - idx) + idx
    return int(prev[m])


_memo = {}


def distance(a, b, K):
    """D = min(lev, K + 1); K + 1 by definition when a window exceeds MAX_WINDOW or the lengths differ by more than K"""
    if len(a) > MAX_WINDOW or len(b) > MAX_WINDOW or abs(len(a) - len(b)) > K:
        return K + 1
    key = (bytes(np.asarray(a, np.uint8)), bytes(np.asarray(b, np.uint8)))
    if key not in _memo:
        _memo[key] = _memo[key[::-1]] = lev(a, b)
    return min(_memo[key], K + 1)


def pair_index(S, t, u):
    return t * S - t * (t + 1) // 2 + (u - t - 1)


def split(D, prm):
    """D: the locus' full matrix [S][S].  Returns (zygosity, c0, c1, n0, n1, cost1, cost2, first) - first[u]: member u belongs to c0"""
    S = len(D)
    K, min_support, min_percent, min_sep, min_gain = prm
    if S < min_support:
        return 0, -1, -1, 0, 0, 0, 0, np.ones(S, bool)
    cost = D.sum(axis=1)
    cstar = int(np.argmin(cost))                         # the smallest c of least cost
    cost1 = int(cost[cstar])
    best = None
    for c0 in range(S):
        for c1 in range(c0 + 1, S):
            first = D[c0] <= D[c1]
            n0 = int(first.sum())
            n1 = S - n0
            cost2 = int(np.minimum(D[c0], D[c1]).sum())
            if min(n0, n1) >= min_support and min(n0, n1) * 100 >= min_percent * S and D[c0, c1] >= min_sep and cost2 * 100 <= cost1 * (100 - min_gain):
                if best is None or (cost2, c0, c1) < best[:3]:
                    best = (cost2, c0, c1, n0, n1, first)
    if best is None:
        return 1, cstar, -1, S, 0, cost1, cost1, np.ones(S, bool)
    cost2, c0, c1, n0, n1, first = best
    return 2, c0, c1, n0, n1, cost1, cost2, first


def members(case):
    """per locus the windows of its entries in list order"""
    read, locus, off, bases = case["read"], case["locus"], case["win_off"], case["win_bases"]
    row = {(int(r), int(l)): k for k, (r, l) in enumerate(zip(read, locus))}
    out = []
    for l in range(case["n_loci"]):
        lo, hi = int(case["support_off"][l]), int(case["support_off"][l + 1])
        rows = [row[(int(case["sup_read"][e]), l)] for e in range(lo, hi)]
        out.append([bases[off[r]:off[r + 1]] for r in rows])
    return out


def sequence_calls(case, prm):
    """A whole input (tests/seq_calls_cases.py: consensus_cases' dict of numpy columns plus `value`) -> the thirteen output columns as numpy, in
    COLUMNS' order.  prm = (max_dist, min_support, min_percent, min_sep, min_gain)"""
    K = prm[0]
    m, S_all = case["n_loci"], len(case["sup_read"])
    value, read = np.zeros(S_all, np.int32), np.zeros(S_all, np.int32)
    allele, dtm = np.zeros(S_all, np.uint8), np.zeros(S_all, np.int32)
    zyg, skipped = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    call, sup, medoid, cost = np.zeros((m, 2), np.int32), np.zeros((m, 2), np.int32), np.full((m, 2), -1, np.int32), np.zeros((m, 2), np.int64)
    pair_off, dist = [0], []
    for l, wins in enumerate(members(case)):
        lo, S = int(case["support_off"][l]), len(wins)
        v, r = case["value"][lo:lo + S], case["sup_read"][lo:lo + S]
        order = np.arange(S)
        if S > MAX_MEMBERS:
            skipped[l] = 1
        else:
            D = np.zeros((S, S), np.int64)
            for t in range(S):
                for u in range(t + 1, S):
                    D[t, u] = D[u, t] = distance(wins[t], wins[u], K)
                    dist.append(D[t, u])
            z, c0, c1, n0, n1, cost1, cost2, first = split(D, prm)
            zyg[l] = z
            if z:
                call[l] = (v[c0], v[c1 if z == 2 else c0])
                sup[l], cost[l] = (n0, n1), (cost1, cost2)
                medoid[l] = (r[c0], r[c1] if z == 2 else -1)
                order = np.concatenate([np.flatnonzero(first), np.flatnonzero(~first)])         # the stable partition
                allele[lo:lo + S] = np.concatenate([np.zeros(n0, np.uint8), np.ones(n1, np.uint8)])
                dtm[lo:lo + S] = [D[u, c0 if first[u] else c1] for u in order]
        value[lo:lo + S], read[lo:lo + S] = v[order], r[order]
        pair_off.append(len(dist))
    return (case["support_off"].astype(np.int64), value, read, allele, zyg, call, sup, cost, medoid, dtm, skipped, np.array(pair_off, np.int64), np.array(dist, np.uint8))
