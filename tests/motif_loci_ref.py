"""The definition of the known-motif locus search (include/mtr_hip.h, "every locus of a motif") in plain Python: the recursion itself, over
tests/motif_search_ref.py's search with its aligner as a parameter.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests import motif_search_ref as ref


def minlen(S: int, G: int) -> int:
    return -(-S // G)


def loci(x, motif_codes, G: int, MM: int, D: int, S: int, R: int, both_strands: bool = True, one=ref.align):
    """-> ([(the nine values in read coordinates, strand)] in ascending start, open) of read codes x against motif codes"""
    x = np.asarray(x, np.uint8)
    out, state, ml = [], {"open": 0}, minlen(S, G)

    def rec(lo, hi, depth):
        if hi - lo < ml:
            return
        if depth == R:
            state["open"] = 1
            return
        hit, strand = ref.search(x[lo:hi], motif_codes, G, MM, D, both_strands=both_strands, one=one)
        if hit[8] < S:
            return
        out.append(((hit[0] + lo, hit[1] + lo) + tuple(hit[2:]), strand))
        rec(lo, lo + hit[0], depth + 1)
        rec(lo + hit[1] + 1, hi, depth + 1)

    rec(0, len(x), 0)
    out.sort(key=lambda h: h[0][0])
    return out, state["open"]


def columns(reads, motifs, G: int, MM: int, D: int, S: int, R: int, both_strands: bool = True, one=ref.align):
    """the columns of Engine.search_motif_loci for a batch, as numpy: loci_off, fields [T, 8], score, ratio, strand, open [n, m]"""
    n, m = len(reads), len(motifs)
    off, f, s, st, op = [0], [], [], [], np.zeros((n, m), np.uint8)
    for i, x in enumerate(reads):
        for j, mo in enumerate(motifs):
            got, op[i, j] = loci(x, mo, G, MM, D, S, R, both_strands, one)
            for hit, strand in got:
                f.append(hit[:8]); s.append(hit[8]); st.append(strand)
            off.append(len(f))
    fields = np.array(f, np.int32).reshape(-1, 8)
    ratio = np.where(fields[:, 2] > 0, fields[:, 4].astype(np.float32) / np.maximum(fields[:, 2], 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return np.array(off, np.int64), fields, np.array(s, np.int32), ratio, np.array(st, np.uint8), op


def three_tracts():
    """flank, (CAG)x15, flank, (CTG)x10, flank, (CAG)x8 with two substitutions, flank: loci on strands 0, 1, 0 for motif CAG, scores (1, 1, 1), S = 12"""
    cag, ctg = ref.codes_of("CAG"), ref.codes_of("CTG")
    third = np.tile(cag, 8)
    third[4] = (third[4] + 1) & 3
    third[16] = (third[16] + 2) & 3
    def flank(k):                                            # A.. T..: under both CAG and CTG one half mismatches throughout, the other two bases in three
        return np.concatenate([np.zeros(k // 2, np.uint8), np.full(k - k // 2, 3, np.uint8)])

    return np.concatenate([flank(23), np.tile(cag, 15), flank(31), np.tile(ctg, 10), flank(18), third, flank(11)]).astype(np.uint8)
