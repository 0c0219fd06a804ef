"""The seeded input set of the unit-search stage tests (tests/test_unit_search_oracle.py) and what the CPU oracle says about it: every search_De_Bruijn_graph call (capture point G2 at level 3), classified by
the k-mer table layout the kernels' tab_build would choose for it.  Nothing here touches a GPU."""
from __future__ import annotations

import functools
import json
import os
import subprocess
import tempfile

import numpy as np

from mtr_amd import synth
from tests.oracle_binding import ORACLE_DIR

# (unit length, copies, flank, reads, error profile): what each shape is there to reach
SHAPES = [
    (3, 25, 60, 4, "nanopore"),        # windows under 100: k = 2..10
    (12, 60, 150, 9, "nanopore"),      # windows under 1000: k = 2..12 (packed up to k = 10, split with keys in LDS for 11 and 12)
    (37, 30, 200, 9, "nanopore"),      # windows of 1000..1400: k = 5..15
    (110, 12, 300, 3, "nanopore"),     # the same with a long unit
    (7, 400, 300, 2, "nanopore"),      # a window beyond 1400 with few distinct keys: the table in global memory, no grouped index
    (150, 20, 300, 2, "nanopore"),     # beyond 1400 with 512 keys or more: the grouped key index (K2_IDX_MIN_KEYS)
    (480, 8, 300, 2, "nanopore"),      # walks that run into MAX_PERIOD
    (300, 20, 200, 1, "sub_heavy"),    # a substitution-heavy read
]
# units that are NEARLY a power of a short string (a short word repeated, a few bases changed): most k-mers occur once per word, so the
# successors' counts tie and the look-ahead runs several levels deep, forward and backward.  (word length, words per unit, changed bases, copies)
NEAR_POWERS = [(5, 6, 2, 40), (4, 8, 2, 40), (6, 5, 2, 40), (7, 4, 1, 60), (3, 11, 2, 30), (5, 9, 3, 40)]
# The two long reads, captured in a run of their own.  A 70 kb repeat under the Nanopore profile: windows of 10 000 to 25 000 positions, every
# k from 5 to 15 in global memory.  (The range finder cuts such a repeat up: its widest pass looks 10 240 positions ahead for a lower minimum.)
WIDE = (50, 1400, 500)
# ... and a read built so that the range finder gives ONE window wider than 65535, whose k = 5, 6 tables cannot be TAB_DIRECT (16-bit counters):
# nine stretches of 9 000 bases that go from copies of one 10-base unit to copies of another, the share of the second growing faster from
# stretch to stretch, so that every boundary is a new minimum of the directional index within reach (10 240) of the one before.
STAIR = (10, 9, 9000, 1000)            # unit length, stretches, bases per stretch, flank

LAYOUTS = ("direct", "packed", "split_lds", "split_global")


def layout(width: int, k: int) -> str:
    """tab_build's rule (mtr_amd/csrc/k2_units.hip.inc), restated: K2_TAB_MAX_WIDTH = 1400, K2_PACK_KEY_BITS = 20"""
    if k <= 6 and width <= 65535:
        return "direct"
    if 2 * k <= 20 and width <= 1400:
        return "packed"
    if width <= 1400:
        return "split_lds"
    return "split_global"


def _near_power_read(rng, word_len, words, changed, copies, flank=150):
    word = rng.randint(0, 4, size=word_len).astype(np.uint8)
    unit = np.tile(word, words)
    for p in rng.choice(len(unit), size=changed, replace=False):
        unit[p] = (unit[p] + rng.randint(1, 4)) % 4
    body = np.tile(unit, copies)
    for p in rng.choice(len(body), size=len(body) // 100, replace=False):     # 1 % substitutions: copies that are not all alike
        body[p] = (body[p] + rng.randint(1, 4)) % 4
    return np.concatenate([rng.randint(0, 4, size=flank).astype(np.uint8), body, rng.randint(0, 4, size=flank).astype(np.uint8)])


@functools.lru_cache(maxsize=None)
def small_reads():
    """the reads of every shape but the wide one, as a tuple of uint8 code arrays"""
    rng = np.random.RandomState(20261018)
    reads = []
    for u, copies, flank, n, profile in SHAPES:
        for _ in range(n):
            reads.append(synth.make_read(rng, u, copies, flank, flank, synth.PROFILES[profile])[0])
    for word_len, words, changed, copies in NEAR_POWERS:
        reads.append(_near_power_read(rng, word_len, words, changed, copies))
    return tuple(reads)


def _stair_read(rng):
    ulen, nseg, seglen, flank = STAIR
    a, b = rng.randint(0, 4, size=ulen).astype(np.uint8), rng.randint(0, 4, size=ulen).astype(np.uint8)
    step = np.array([(j + 1) * (j + 2) / 2 for j in range(nseg - 1)])
    share_b = np.concatenate([[0.0], np.cumsum(step / step.sum())])               # of the second unit, per stretch: 0 .. 1
    parts = [rng.randint(0, 4, size=flank).astype(np.uint8)]
    for j in range(nseg):
        t = np.arange(seglen // ulen)
        is_b = np.floor((t + 1) * share_b[j] + 1e-9) > np.floor(t * share_b[j] + 1e-9)      # evenly spread
        parts.append(np.where(is_b[:, None], b[None, :], a[None, :]).reshape(-1).astype(np.uint8))
    parts.append(rng.randint(0, 4, size=flank).astype(np.uint8))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def wide_reads():
    u, copies, flank = WIDE
    return (synth.make_read(np.random.RandomState(20261019), u, copies, flank, flank)[0], _stair_read(np.random.RandomState(1)))


def capture_g2(reads, level=3):
    """the oracle's capture of `reads` at `level`: its G2 lines as dicts in make_golden_l2.py's form (rd = index of the read)"""
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)
    with tempfile.TemporaryDirectory() as tmp:
        fa, cap = os.path.join(tmp, "in.fa"), os.path.join(tmp, "cap.jsonl")
        synth.write_fasta(fa, [(str(i), c) for i, c in enumerate(reads)])
        subprocess.run([os.path.join(ORACLE_DIR, "mtr_oracle_cli"), "-l", str(level), "-C", cap, fa], check=True, stdout=subprocess.DEVNULL)
        rd, out = -1, []
        with open(cap) as fh:
            for line in fh:
                ev = json.loads(line)
                if ev["t"] == "G1":
                    rd += 1
                elif ev["t"] == "G2":
                    out.append(g2_line(rd, ev))
    return out


FIELDS = ("period", "rep_start", "rep_end", "repeat_len", "copies", "mat", "mis", "ins", "del")


def g2_line(rd, ev):
    rr = ev["rr"]
    d = {"rd": rd, "qs": ev["qs"], "qe": ev["qe"], "k": ev["k"], "found": ev["found"]}
    d.update({f: rr[f] for f in FIELDS})
    d["unit"] = rr["unit"]
    return d


@functools.lru_cache(maxsize=None)
def oracle_g2_small():
    return tuple(capture_g2(small_reads()))


@functools.lru_cache(maxsize=None)
def oracle_g2_wide():
    return tuple(capture_g2(wide_reads()))


def regime_counts(events):
    """per layout: searches that found a unit, found ones with period > 10, searches that found none"""
    cnt = {name: {"found": 0, "found_period_gt_10": 0, "not_found": 0} for name in LAYOUTS}
    for g in events:
        c = cnt[layout(g["qe"] - g["qs"] + 1, g["k"])]
        if g["found"]:
            c["found"] += 1
            c["found_period_gt_10"] += g["period"] > 10
        else:
            c["not_found"] += 1
    return cnt


def assert_every_regime_is_reached(events):
    """The floors that keep the stage tests from passing empty: conditions on the ORACLE's events, not measurements."""
    cnt = regime_counts(events)
    for name in LAYOUTS:
        assert cnt[name]["found"] >= 40, (name, cnt)
    assert cnt["split_global"]["found_period_gt_10"] >= 20, cnt
    assert cnt["split_lds"]["found"] >= 20, cnt
    assert any(g["found"] and g["qe"] - g["qs"] + 1 > 65535 and g["k"] <= 6 for g in events), "no found search of k <= 6 in a window wider than 65535"
    for name in ("packed", "split_lds", "split_global"):
        assert cnt[name]["not_found"] >= 10, (name, cnt)
    return cnt


# (found, not found) per layout over both captures: what DESIGN.md quotes; deterministic for the seeded set (test_unit_search_oracle.py)
DOCUMENTED_COUNTS = {"direct": (1505, 20825), "packed": (390, 17430), "split_lds": (105, 117), "split_global": (159, 17)}
