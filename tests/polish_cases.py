"""Crafted polish_repeat calls (consensus.c:610-704) for tests/test_polish_plan_host.py and tests/test_gpu_polish.py.

A case is a read, a repeat [rep_start, rep_end] in it, k, a unit and its node frequencies.  The repeat is a variant of the unit, copy after
copy: where the variant has another base than the unit (sub), a base the unit lacks (ins) or lacks a base of the unit (del), and the node
frequencies around that place are 1, the walk finds the repeat's k-mers more frequent than the unit's own and alters the unit there.  What a
case was made for is in its `want`: the tests assert it on the walk over every position, so a case cannot quietly stop exercising its path.
  altered / unchanged       the walk altered a position / left the unit as it was
  undefined                 it altered position 0 (the reference reads int_unit[-1] there)
  flag_in_first_k           a flagged position lies inside the first k - 1 positions (the `0 <= j - i` cut of suspicious())
  dirty_flag                a flagged position is met while the node is not the unit's own (two flags closer than k)
  longer / shorter          the polished unit has more / fewer bases (an alteration with step 0 / with step 2)
  overflow                  the output outgrew MAX_PERIOD and the unit stays (jr < 0)
  no_table                  period <= k or no flagged position: the table is not built"""
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

from mtr_amd import synth

MAX_PERIOD = 500
ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
B2C = {c: i for i, c in enumerate("ACGT")}


@functools.lru_cache(maxsize=None)
def oracle_g3p(workload="headline2k", n_reads=300, seed=2):
    """-> (reads, calls): every polish_repeat call of the CPU oracle on these reads (its G3p capture lines, level 1), in the oracle's order:
    dicts with rd (index of the read), rep_start, rep_end, k, unit, score, out (codes 0..3)"""
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)
    reads = [c for _, c in synth.make_reads(workload, n_reads, seed)]
    calls = []
    with tempfile.TemporaryDirectory() as tmp:
        fa, cap = os.path.join(tmp, "in.fa"), os.path.join(tmp, "cap.jsonl")
        synth.write_fasta(fa, [(str(i), c) for i, c in enumerate(reads)])
        subprocess.run([os.path.join(ORACLE_DIR, "mtr_oracle_cli"), "-l", "1", "-C", cap, fa], check=True, stdout=subprocess.DEVNULL)
        rd = -1
        with open(cap) as fh:
            for line in fh:
                if line.startswith('{"t":"G1"'):
                    rd += 1
                elif line.startswith('{"t":"G3p"'):
                    ev = json.loads(line)
                    calls.append({"rd": rd, "rep_start": ev["rep_start"], "rep_end": ev["rep_end"], "k": ev["k"],
                                  "unit": np.array([B2C[ch] for ch in ev["in"]], np.uint8), "score": np.array(ev["in_score"], np.int32),
                                  "out": np.array([B2C[ch] for ch in ev["out"]], np.uint8)})
    return reads, calls


def pack(codes):
    """2 bits a base, first base in the top bits of word 0, two zero words behind the last"""
    codes = np.asarray(codes, np.uint8)
    pk = np.zeros(len(codes) // 16 + 3, np.uint32)
    for i, c in enumerate(codes):
        pk[i >> 4] |= np.uint32(int(c) << (30 - 2 * (i & 15)))
    return pk


def _variant(unit, edits, rng):
    out = []
    ed = {p: kind for p, kind in edits}
    for p, b in enumerate(unit):
        kind = ed.get(p)
        if kind == "del":
            continue
        if kind == "ins":
            out.append((int(b) + 1 + rng.randint(3)) % 4)
        out.append((int(b) + 1 + rng.randint(3)) % 4 if kind == "sub" else int(b))
    return out


def make(name, k, period, edits, seed, want, copies=6, lead=7, tail=5, low_all=False, low_extra=()):
    rng = np.random.RandomState(seed)
    unit = rng.randint(0, 4, size=period).astype(np.uint8)
    var = _variant(unit, edits, rng)
    read = list(rng.randint(0, 4, size=lead)) + var * copies + list(rng.randint(0, 4, size=tail))
    rep_start, rep_end = lead, lead + len(var) * copies - 1
    score = np.full(period, 1 if low_all else 3, np.int32)
    for p, _ in list(edits) + [(q, None) for q in low_extra]:
        score[max(0, p - k):min(period, p + k + 1)] = 1
    return {"name": name, "edits": list(edits), "read": np.asarray(read, np.uint8), "rep_start": rep_start, "rep_end": rep_end, "k": k, "unit": unit,
            "score": score, "want": set(want)}


def crafted():
    c = []
    # a flag at j = 0 needs (k - 1) * 0.8 < 1, that is k = 2: the window of suspicious() holds position 0 alone
    c.append(make("flag_at_0_k2", 2, 6, [(0, "sub")], 4, {"altered", "undefined", "flag_in_first_k", "longer"}))
    c.append(make("flag_at_0_k2_step_0_for_ever", 2, 6, [(0, "sub")], 3, {"altered", "undefined", "overflow"}))        # 495 int_unit[-1] reads
    # inside the first k - 1 positions the window is cut: position j is flagged only if j + 1 > 0.8 (k - 1), for k = 7 from j = 4
    c.append(make("flag_inside_first_k", 7, 63, [(4, "sub")], 1, {"altered", "flag_in_first_k"}))
    # low frequencies at the unit's first six positions only: the cut window of position 5 holds six of them, 6 <= 0.8 * 9, no flag
    c.append(make("low_start_below_the_cut", 10, 64, [(3, "sub")], 19, {"unchanged", "no_table"}))
    c[-1]["score"][:] = 3
    c[-1]["score"][:6] = 1
    c.append(make("two_flags_closer_than_k", 10, 64, [(30, "sub"), (33, "sub")], 2, {"altered", "dirty_flag"}))
    c.append(make("two_flags_closer_than_k_split_table", 12, 129, [(70, "sub"), (72, "sub")], 4, {"altered", "dirty_flag"}))
    c.append(make("step_0", 7, 65, [(40, "ins")], 5, {"altered", "longer"}))
    c.append(make("step_2", 7, 65, [(40, "del")], 6, {"altered", "shorter"}))
    c.append(make("step_0_k11", 11, 128, [(100, "ins")], 7, {"altered", "longer"}))
    c.append(make("step_2_k6_direct_table", 6, 128, [(17, "del")], 8, {"altered", "shorter"}))
    c.append(make("overflow_499", 10, 499, [(100, "ins"), (300, "ins")], 9, {"altered", "overflow"}, copies=4))
    c.append(make("unit_499_unflagged_middle", 10, 499, [(250, "sub")], 10, {"altered"}, copies=4))
    c.append(make("period_equals_k", 6, 6, [(2, "sub")], 11, {"unchanged", "no_table"}, low_all=True))
    c.append(make("period_below_k", 10, 6, [(2, "sub")], 12, {"unchanged", "no_table"}, low_all=True))
    c.append(make("period_k_plus_1", 6, 7, [(3, "sub")], 13, {"altered"}, low_all=True, copies=12))
    c.append(make("no_flag", 10, 128, [(60, "sub")], 14, {"unchanged", "no_table"}, low_extra=()))
    c[-1]["score"][:] = 3
    c.append(make("flags_that_alter_nothing", 10, 129, [], 15, {"unchanged"}, low_extra=(20, 64, 100)))
    c.append(make("all_low_k2_unit_6", 2, 6, [], 16, {"altered", "overflow"}, low_all=True, copies=10))
    c.append(make("flag_at_word_ends", 7, 129, [(63, "sub"), (64, "sub"), (128, "sub")], 17, {"altered", "dirty_flag"}))
    c.append(make("all_low_k12", 12, 65, [(10, "sub"), (50, "del")], 18, {"altered"}, low_all=True))
    return c
