"""The window structure in plain Python, written from the definition in include/mtr_hip.h ("window structure") and sharing nothing with
mtr_amd/csrc/window_structure.h: the full matrix with one stored predecessor per cell, every row filled by iterating over its columns until
nothing changes (the fixpoint itself - that two sweeps reach it is what the library claims, not what this assumes), then one walk back from the
end that counts copies, matches and entries and notes what kinds of step it took.  Reference for the CPU and the GPU tests."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

MAX_SEGMENTS, MAX_WINDOW = 4, 16384
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
START = -1                    # the state before any motif base
NONE = None                   # minus infinity


class Structure(NamedTuple):
    score: int
    seg: list                 # [4][4]: start, end, copies, matches
    ratio: np.float32
    skipped: int
    steps: set                # the kinds of step on the walk back, and the ties met (see structure())


def as_motifs(structure):
    return [structure] if isinstance(structure, str) else list(structure)


def limit_ok(motifs) -> bool:
    S, W = len(motifs), sum(len(m) for m in motifs)
    return all(len(m) >= 1 for m in motifs) and ((1 <= S <= 2 and W <= 32) or (1 <= S <= 4 and W <= 16))


def codes(s) -> list:
    return [CODE[c] for c in s] if isinstance(s, str) else [int(c) for c in s]


def structure(motifs, window, gain=1, mismatch=1, indel=1) -> Structure:
    motifs = as_motifs(motifs)
    assert limit_ok(motifs), motifs
    y = codes(window)
    n, S = len(y), len(motifs)
    zeros = [[0] * 4 for _ in range(4)]
    if n > MAX_WINDOW:
        return Structure(0, zeros, np.float32(0), 1, set())
    if n == 0:
        return Structure(0, zeros, np.float32(0), 0, set())
    G, MM, D = gain, mismatch, indel
    m, seg, first, last = [], [], [], []
    for s, mo in enumerate(motifs):
        first.append(len(m))
        m += codes(mo)
        seg += [s] * len(mo)
        last.append(len(m) - 1)
    W = len(m)
    preds = []
    for c in range(W):
        s = seg[c]
        preds.append([c - 1] if c != first[s] else [last[t] for t in range(s - 1, -1, -1)] + [START, last[s]])

    def candidates(H, i, c):
        """(value, kind, predecessor) in the definition's order"""
        out = []
        if i >= 1:
            for p in preds[c]:
                v = H[i - 1][p]
                if v is not NONE:
                    out.append((v + (G if y[i - 1] == m[c] else -MM), "sub", p))
            if H[i - 1][c] is not NONE:
                out.append((H[i - 1][c] - D, "up", c))
        for p in preds[c]:
            v = H[i][p]
            if v is not NONE:
                out.append((v - D, "left", p))
        return out

    H, back = [], []                      # H[i][c] with H[i][START] at index -1 (the list's last element); back[i][c] = (kind, p, tie notes)
    for i in range(n + 1):
        H.append([NONE] * W + [-D * i])
        back.append([None] * W)
        sweeps, changed = 0, True
        while changed:
            changed = False
            sweeps += 1
            for c in range(W):
                cand = candidates(H, i, c)
                if not cand:
                    continue
                best = max(v for v, _, _ in cand)
                kind, p = next((k, q) for v, k, q in cand if v == best)
                ties = {k for v, k, _ in cand if v == best}
                if H[i][c] != best or back[i][c] is None or back[i][c][:2] != (kind, p):
                    changed = True
                H[i][c], back[i][c] = best, (kind, p, ties)
        assert sweeps <= 2 * W + 2, "the row did not settle"

    ends = [last[s] for s in range(S - 1, -1, -1)] + [START]
    score = max(H[n][e] for e in ends)
    e = next(e for e in ends if H[n][e] == score)
    steps = set()
    if e == START:
        steps.add("end:START")
    if sum(1 for x in ends if H[n][x] == score) > 1:
        steps.add("end:tie")
    copies, matches, entry = [0] * S, [0] * S, [0] * S
    i, c = n, e
    while c != START:
        kind, p, ties = back[i][c]
        s = seg[c]
        where = "START" if p == START else "wrap" if (c == first[s] and p == last[s]) else "inside" if c != first[s] else "outside"
        steps.add(kind if kind == "up" else f"{kind}:{where}")
        if {"sub", "up"} <= ties:
            steps.add("tie:sub=up")
        if kind == "up" and "left" in ties:
            steps.add("tie:up=left")
        if kind == "left" and where == "inside":              # the run-on: lefts all the way back to a first column that took the wrap's left
            q = p
            while q != first[s] and back[i][q][0] == "left":
                q = back[i][q][1]
            if q == first[s] and back[i][q][:2] == ("left", last[s]):
                steps.add("left:run-on")
        if kind == "left" and i == 0 and c == first[s]:
            steps.add("left:row0-entry")
        if kind != "up":
            if c == last[s]:
                copies[s] += 1
            if kind == "sub" and y[i - 1] == m[c]:
                matches[s] += 1
            if c == first[s] and where != "wrap":
                entry[s] = i - 1 if kind == "sub" else i
        if kind == "sub":
            i, c = i - 1, p
        elif kind == "up":
            i -= 1
        else:
            c = p
    out = [[0] * 4 for _ in range(4)]
    nxt = n
    for s in range(S - 1, -1, -1):
        if copies[s] > 0:
            out[s] = [entry[s], nxt, copies[s], matches[s]]
            nxt = entry[s]
        else:
            out[s] = [nxt, nxt, 0, 0]
    return Structure(int(score), out, np.float32(sum(matches)) / np.float32(n), 0, steps)


def columns(structures, windows, which, gain=1, mismatch=1, indel=1):
    """the call's four columns as numpy arrays: seg [N, 4, 4] int32, score int32, ratio float32, skipped uint8"""
    N = len(windows)
    seg, score, ratio, skipped = np.zeros((N, 4, 4), np.int32), np.zeros(N, np.int32), np.zeros(N, np.float32), np.zeros(N, np.uint8)
    for w in range(N):
        r = structure(structures[which[w]], windows[w], gain, mismatch, indel)
        seg[w], score[w], ratio[w], skipped[w] = r.seg, r.score, r.ratio, r.skipped
    return seg, score, ratio, skipped
