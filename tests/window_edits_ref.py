"""The window edits in plain Python, written from the definition in include/mtr_hip.h ("window edits") and sharing nothing with
mtr_amd/csrc/window_edits.h: the full matrix, every row filled by iterating over its columns until nothing changes, ONE stored predecessor per
cell - the first candidate of the definition's order that attains the maximum -, then the path from the end back to START, read forward: the copy
index counted step by step, every edit listed as it is met.  Reference for the CPU and the GPU tests."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

MAX_WINDOW = 16384
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
START = "START"
SUB, INS, DEL = 0, 1, 2


class Edits(NamedTuple):
    edits: list               # [pos, segment, copy, column, kind, base] per edit, in path order
    seg: list                 # [4][4]: start, end, copies, matches
    score: int
    skipped: int
    path: list                # (i, c, step, predecessor) per step, forward; c a flat column


def _codes(s):
    return [CODE[ch] for ch in s] if isinstance(s, str) else [int(v) for v in s]


def edits(motifs, window, gain=1, mismatch=1, indel=1) -> Edits:
    motifs = [motifs] if isinstance(motifs, str) else list(motifs)
    S, W = len(motifs), sum(len(mo) for mo in motifs)
    assert all(len(mo) >= 1 for mo in motifs) and ((1 <= S <= 2 and W <= 32) or (1 <= S <= 4 and W <= 16)), motifs
    y = _codes(window)
    n = len(y)
    none = [[0] * 4 for _ in range(4)]
    if n > MAX_WINDOW:
        return Edits([], none, 0, 1, [])
    if n == 0:
        return Edits([], none, 0, 0, [])
    m, seg_of, first, last = [], [], [], []
    for s, mo in enumerate(motifs):
        first.append(len(m))
        m.extend(_codes(mo))
        seg_of.extend([s] * len(mo))
        last.append(len(m) - 1)

    def predecessors(c):
        s = seg_of[c]
        return [c - 1] if c != first[s] else [last[t] for t in range(s - 1, -1, -1)] + [START, last[s]]

    H = [dict() for _ in range(n + 1)]          # H[i][c], c a column or START; a missing key is minus infinity
    back = [dict() for _ in range(n + 1)]       # back[i][c] = (step, predecessor)
    for i in range(n + 1):
        H[i][START] = -indel * i
        while True:
            changed = False
            for c in range(W):
                cand = []                        # (value, step, predecessor) in the definition's order: subs, up, lefts
                if i >= 1:
                    cand += [(H[i - 1][p] + (gain if y[i - 1] == m[c] else -mismatch), "sub", p) for p in predecessors(c) if p in H[i - 1]]
                    if c in H[i - 1]:
                        cand.append((H[i - 1][c] - indel, "up", c))
                cand += [(H[i][p] - indel, "left", p) for p in predecessors(c) if p in H[i]]
                if not cand:
                    continue
                best = max(v for v, _, _ in cand)
                step, p = next((k, q) for v, k, q in cand if v == best)
                if H[i].get(c) != best or back[i].get(c) != (step, p):
                    H[i][c], back[i][c], changed = best, (step, p), True
            if not changed:
                break
    ends = [last[s] for s in range(S - 1, -1, -1)] + [START]
    score = max(H[n][e] for e in ends)
    end = next(e for e in ends if H[n][e] == score)
    path = []
    i, c = n, end
    while c != START:
        step, p = back[i][c]
        path.append((i, c, step, p))
        if step == "sub":
            i, c = i - 1, p
        elif step == "up":
            i -= 1
        else:
            c = p
    path.reverse()
    landings, copies, matches, entry = [0] * S, [0] * S, [0] * S, [0] * S
    out = []
    for i, c, step, p in path:
        s = seg_of[c]
        if step != "up":
            if c == first[s]:
                landings[s] += 1
                if p != last[s]:
                    entry[s] = i - 1 if step == "sub" else i
            if c == last[s]:
                copies[s] += 1
        copy, column = landings[s] - 1, c - first[s]
        if step == "sub":
            if y[i - 1] == m[c]:
                matches[s] += 1
            else:
                out.append([i - 1, s, copy, column, SUB, y[i - 1]])
        elif step == "up":
            out.append([i - 1, s, copy, column, INS, y[i - 1]])
        else:
            out.append([i, s, copy, column, DEL, m[c]])
    assert landings == copies, (landings, copies)          # only whole copies exist
    seg = [[0] * 4 for _ in range(4)]
    nxt = n
    for s in range(S - 1, -1, -1):
        if copies[s] > 0:
            seg[s] = [entry[s], nxt, copies[s], matches[s]]
            nxt = entry[s]
        else:
            seg[s] = [nxt, nxt, 0, 0]
    return Edits(out, seg, int(score), 0, path)


def invariants_hold(motifs, e: Edits) -> bool:
    """per segment: copies * U == matches + substitutions + deletions, and end - start == matches + substitutions + insertions"""
    motifs = [motifs] if isinstance(motifs, str) else list(motifs)
    for s, mo in enumerate(motifs):
        k = [sum(1 for row in e.edits if row[1] == s and row[4] == kind) for kind in (SUB, INS, DEL)]
        start, end, copies, matches = e.seg[s]
        if copies * len(mo) != matches + k[SUB] + k[DEL] or end - start != matches + k[SUB] + k[INS]:
            return False
    return True


def columns(structures, windows, which, gain=1, mismatch=1, indel=1):
    """the call's five columns as numpy arrays: off int64 [N + 1], edits int32 [T, 6], seg int32 [N, 4, 4], score int32 [N], skipped uint8 [N]"""
    N = len(windows)
    off, rows = np.zeros(N + 1, np.int64), []
    seg, score, skipped = np.zeros((N, 4, 4), np.int32), np.zeros(N, np.int32), np.zeros(N, np.uint8)
    for w in range(N):
        e = edits(structures[which[w]], windows[w], gain, mismatch, indel)
        rows += e.edits
        off[w + 1] = len(rows)
        seg[w], score[w], skipped[w] = e.seg, e.score, e.skipped
    return off, np.array(rows, np.int32).reshape(-1, 6), seg, score, skipped
