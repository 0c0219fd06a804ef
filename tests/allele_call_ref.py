"""Allele calls in numpy, written straight from the definition in include/mtr_hip.h ("allele calls"): the supporting rows, np.lexsort by
(value, read), then every split's sad by explicit sums - no prefix trick.  Genotypes' columns as numpy in, AlleleCalls' columns as numpy out.
It also says WHY: per locus how many splits each admissibility condition alone refused, and whether the least cost2 was a tie, so that the
tests can show from the reference alone that their inputs are not degenerate."""
import numpy as np

CONDITIONS = ("distinct", "support", "percent", "sep")


def med(v, i, j):
    return int(v[i + (j - i - 1) // 2])


def sad(v, i, j):
    m = med(v, i, j)
    return int(np.abs(np.asarray(v[i:j], np.int64) - m).sum())


def split(v, min_support, min_percent, min_sep):
    """v: the sorted values of one locus -> (zygosity, call, call_support, cost, k, why); k = 0 without a split; why: {"tie": bool, and per
    condition the number of splits that this condition refused and every other one admitted}"""
    S = len(v)
    why = dict.fromkeys(CONDITIONS, 0)
    why["tie"] = False
    if S < max(min_support, 1):
        return 0, (0, 0), (0, 0), (0, 0), 0, why
    cost1, best = sad(v, 0, S), None
    for k in range(1, S):
        small = min(k, S - k)
        ok = {"distinct": int(v[k - 1]) < int(v[k]), "support": small >= min_support, "percent": small * 100 >= min_percent * S,
              "sep": med(v, k, S) - med(v, 0, k) >= min_sep}
        failed = [c for c in CONDITIONS if not ok[c]]
        if len(failed) == 1:
            why[failed[0]] += 1
        if failed:
            continue
        cost2 = sad(v, 0, k) + sad(v, k, S)
        if best is None or cost2 < best[0]:
            best, why["tie"] = (cost2, k), False
        elif cost2 == best[0]:
            why["tie"] = True
    if best is None:
        return 1, (med(v, 0, S),) * 2, (S, 0), (cost1, cost1), 0, why
    k = best[1]
    return 2, (med(v, 0, k), med(v, k, S)), (k, S - k), (cost1, best[0]), k, why


def supporting(spanning, window, fields, ratio, measure, min_ratio):
    """-> (supports [n, m] bool, value [n, m] int64); a supporting row of negative value raises ValueError naming the row"""
    length = window[:, :, 1].astype(np.int64) - window[:, :, 0].astype(np.int64)
    ok = (spanning == 1) & ((window[:, :, 1] == window[:, :, 0]) | (ratio.astype(np.float32) >= np.float32(min_ratio)))
    value = fields[:, :, 3].astype(np.int64) if measure == 0 else length
    bad = np.argwhere(ok & (value < 0))
    if len(bad):
        raise ValueError(f"row {int(bad[0][0]) * spanning.shape[1] + int(bad[0][1])} supports its locus with a negative value")
    return ok, value


def call_alleles(gt, measure=0, min_ratio=0.0, min_support=2, min_percent=20, min_sep=1):
    """gt: Genotypes' seven columns (or anything with spanning, window, fields, ratio) as numpy -> (AlleleCalls' eight columns, why per locus)"""
    spanning, window, fields, ratio = (np.asarray(getattr(gt, c)) for c in ("spanning", "window", "fields", "ratio"))
    n, m = spanning.shape
    ok, value = supporting(spanning, window, fields, ratio, measure, min_ratio)
    off = np.zeros(m + 1, np.int64)
    vals, reads, allele, whys = [], [], [], []
    zyg, call, sup, cost = np.zeros(m, np.uint8), np.zeros((m, 2), np.int32), np.zeros((m, 2), np.int32), np.zeros((m, 2), np.int64)
    for l in range(m):
        rd = np.nonzero(ok[:, l])[0]
        v = value[rd, l]
        order = np.lexsort((rd, v))
        rd, v = rd[order], v[order]
        zyg[l], call[l], sup[l], cost[l], k, why = split(v, min_support, min_percent, min_sep)
        off[l + 1] = off[l] + len(v)
        vals.append(v.astype(np.int32)); reads.append(rd.astype(np.int32)); whys.append(why)
        allele.append((np.arange(len(v)) >= k).astype(np.uint8) if k > 0 else np.zeros(len(v), np.uint8))
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, t)      # noqa: E731
    return (off, cat(vals, np.int32), cat(reads, np.int32), cat(allele, np.uint8), zyg, call, sup, cost), whys
