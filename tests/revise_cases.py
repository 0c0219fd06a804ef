"""Seeded cases for the revision rounds (revise_representative_unit, consensus.c:1048-1087): records and units of the test's choosing (test
infrastructure only).

A task is what the batch path hands to a revision: a read, the 13 scalar fields of a record (rep_start, rep_end, repeat_len, period, copies, mat, mis,
ins, del, k, G, MM, D), the record's unit and the unit's node frequencies.  The reads are tests/dp_pass_cases.py windows of U x copies + 3 rows; the unit
is the window's true unit or a corruption of it; the record is the better of Oracle.wrap_dp under (1,1,3) and (1,3,1) for THAT unit, as wrap_around_DP
chooses.  Tasks keeps the reads of a test's tasks and makes the tuples Engine.test_revise takes.  tests/test_revise_cases_ref.py shows from the oracle
alone that every outcome of a round occurs in quantity; tests/test_gpu_revise.py runs the tasks on the kernels.  docs/revision_tests.md says what each
set is for.
"""
from __future__ import annotations

import numpy as np

from tests import dp_pass_cases as dc

# either side of every columns-per-lane border of a 16-lane pass that admits coverage >= 5; 129 .. 260 take revise_sub / dp_sub by themselves
# (ST_QUMAX = 128), 227 and 260 with their votes beyond what the per-read kernel's LDS holds (9 (U + 1) words <= K2_TAB_CAP: U <= 226)
UNITS = (6, 7, 16, 17, 32, 33, 64, 65, 127, 128, 129, 200, 226, 227, 260)
COPIES = (5, 6, 12, 20, 21)
MORE_UNITS = (48, 49, 80, 81, 96, 97, 112, 113)          # the remaining borders of the 16-lane passes, with 5 and 12 copies
KINDS = ("perfect", "noisy")
CORRUPTIONS = ("exact", "sub", "del", "ins", "del2", "double")
K_CYCLE = (5, 2, 7, 15, 10, 3)
QS_CYCLE = (0, 1, 15, 16, 33)
MAX_PERIOD = 500


class Task:
    __slots__ = ("read", "rr", "unit", "score", "tag", "U0", "copies", "kind", "how")

    def __init__(self, read, rr, unit, score, tag="", U0=0, copies=0, kind="", how=""):
        self.read, self.rr, self.unit, self.score = read, tuple(int(v) for v in rr), np.asarray(unit, np.uint8), np.asarray(score, np.int32)
        self.tag, self.U0, self.copies, self.kind, self.how = tag, U0, copies, kind, how
        assert len(self.rr) == 13 and len(self.unit) == len(self.score)     # (rr[3] is the unit's length in every task but those made to be refused)

    @property
    def U(self):
        return len(self.unit)

    @property
    def rows(self):
        return self.rr[1] - self.rr[0] + 1

    @property
    def coverage(self):
        return self.rr[2] // self.rr[3]

    def with_rr(self, tag, **fields):
        names = ("rep_start", "rep_end", "repeat_len", "period", "copies", "mat", "mis", "ins", "del_", "k", "G", "MM", "D")
        rr = list(self.rr)
        for n, v in fields.items():
            rr[names.index(n)] = v
        return Task(self.read, rr, self.unit, self.score, tag, self.U0, self.copies, self.kind, self.how)

    def with_unit(self, unit, score, tag):
        rr = list(self.rr)
        rr[3] = len(unit)
        return Task(self.read, rr, unit, score, tag, self.U0, self.copies, self.kind, self.how)

    def __repr__(self):
        return f"<{self.tag} {self.kind} {self.how} U0={self.U0}x{self.copies} U={self.U} rr={self.rr}>"


def eligible(t: Task) -> bool:
    """mtr_amd/csrc/revise_task.h for a task of these sets (WrapDPsize is out of their reach)"""
    rs, re, rl, U = t.rr[:4]
    return (6 <= U <= 499 and 0 <= rs <= re <= len(t.read) and min(t.rr[5:9]) >= 0 and sum(t.rr[5:9]) > 0 and rl > 0 and 5 <= rl // U <= 20
            and 2 <= t.rr[9] <= 15)


def corrupt(rng, m: np.ndarray, how: str) -> np.ndarray:
    U = len(m)
    p = int(rng.randint(1, U - 2))
    if how == "exact":
        return m.copy()
    if how == "sub":
        out = m.copy()
        out[p] = (int(out[p]) + 1 + rng.randint(0, 3)) & 3
        return out
    if how == "del":
        return np.delete(m, p)
    if how == "ins":
        return np.insert(m, p, rng.randint(0, 4)).astype(np.uint8)
    if how == "del2":
        return np.delete(m, [p, p + 1])
    if how == "double":
        return np.concatenate([m, m])
    raise ValueError(how)


def record(orc, read, qs, qe, unit, k):
    """wrap_around_DP (wrap_around_DP.c:357-429) of `unit` over rows qs+1 .. qe+1: (1,1,3) then (1,3,1), the strictly better float ratio wins.
    None for an empty alignment."""
    best, best_ratio = None, np.float32(-1)
    for (G, MM, D) in dc.SETS2:
        rs, re, rl, cp, mat, mis, ins, dl = (int(v) for v in orc.wrap_dp(read, qs, qe, unit, G, MM, D))
        tot = mat + mis + ins + dl
        if tot <= 0 or rl <= 0:
            continue
        ratio = np.float32(mat) / np.float32(tot)
        if best_ratio < ratio:
            best_ratio, best = ratio, (rs, re, rl, len(unit), cp, mat, mis, ins, dl, k, G, MM, D)
    return best


def plain_scores(rng, U):
    """node frequencies of 2 and more: polish_repeat flags nothing, the unit goes to the rounds as it is"""
    return rng.randint(2, 30, size=U).astype(np.int32)


def grid(orc, seed: int = 5, units=UNITS, copies=COPIES):
    """every unit length x copies x kind: one read each, and on it one task per corruption of its unit (the doubled one while 2 U < 500).  Placement
    cycles: windows that start on base 1 of their read (qs = 0; the first read of the list is one), one read in four without a base behind the window."""
    rng = np.random.RandomState(seed)
    out, n = [], 0
    for U in units:
        for cp in copies:
            for kind in KINDS:
                c = dc.make_case(rng, U, U * cp + 3, QS_CYCLE[n % len(QS_CYCLE)], kind, tail=n % 4, tag="grid")
                for how in CORRUPTIONS:
                    if how == "double" and 2 * U >= MAX_PERIOD:
                        continue
                    unit = corrupt(rng, c.unit, how)
                    rr = record(orc, c.read, c.qs, c.qe, unit, K_CYCLE[n % len(K_CYCLE)])
                    if rr is not None:
                        out.append(Task(c.read, rr, unit, plain_scores(rng, len(unit)), "grid", U, cp, kind, how))
                n += 1
    return out


def end_tasks(orc, seed: int = 6, units=(7, 33, 129, 17)):
    """records with rep_end = L: a clean repeat cut in front of a base 0 of its unit, searched with the window's last row on org[L] (query_end = L - 1) -
    org[L] = 0 continues the repeat, the alignment ends on it, as a batch's does where a repeat runs to the end of its read.  The first of
    them also starts on base 0 of its record (rep_start = 0: the base in front of the window continues the repeat leftwards).  Their reads go last."""
    rng = np.random.RandomState(seed)
    out = []
    for n, U in enumerate(units):
        m = dc.make_unit(rng, U, "perfect")
        m[U // 2] = 0
        rows = U * 7 + 3
        w = np.array([m[(U // 2 + 1 + i) % U] for i in range(rows)], np.uint8)
        j = max(i for i in range(rows) if w[i] == 0)                      # the window's bases w[:j]; w[j] = 0 is org[L]
        qs = 0 if n == 0 else 9
        front = rng.randint(0, 4, size=qs + 1).astype(np.uint8)
        front[-1] = m[(U // 2) % U]                                        # the base in front of the window continues the repeat
        read = np.concatenate([front, w[:j]])
        unit = corrupt(rng, m, "sub" if n & 1 else "exact")
        rr = record(orc, read, qs, len(read) - 1, unit, 5)
        assert rr is not None and rr[1] == len(read), (U, rr, len(read))
        t = Task(read, rr, unit, plain_scores(rng, len(unit)), "ends on L", U, 7, "perfect", "sub" if n & 1 else "exact")
        if n == 0:                                                         # one base more to the left: the record a search window starting there gives
            t = t.with_rr("starts on 0, ends on L", rep_start=0, repeat_len=rr[2] + 1, mat=rr[5] + 1)
        out.append(t)
    return out


def polish_tasks(orc, seed: int = 7):
    """node frequencies of 1 over a run of 2 k positions (k = 3, 5, 8) around a corruption of the unit, 5 elsewhere: polish_repeat walks the run
    (every position of it is flagged once k - 1 ones lie behind it) and puts the repeat's own k-mers back where it finds better ones"""
    rng = np.random.RandomState(seed)
    out = []
    for U in (17, 33, 48, 65, 128, 129):
        for cp in (6, 12):
            for kind in KINDS:
                c = dc.make_case(rng, U, U * cp + 3, 1 + rng.randint(0, 20), kind, tail=rng.randint(0, 3), tag="polish")
                for k in (3, 5, 8):
                    for how in ("sub", "del", "ins"):
                        unit = corrupt(rng, c.unit, how)
                        rr = record(orc, c.read, c.qs, c.qe, unit, k)
                        if rr is None:
                            continue
                        score = np.full(len(unit), 5, np.int32)
                        at = int(rng.randint(0, len(unit) - 2 * k + 1))
                        score[at:at + 2 * k] = 1
                        out.append(Task(c.read, rr, unit, score, f"polish k={k}", U, cp, kind, how))
    return out


class Tasks:
    """the reads of a test's tasks (in the order first used, `last` reads moved to the end) and the engine's tuples"""

    def __init__(self):
        self.reads, self.tasks, self.read_of = [], [], []

    def add(self, t: Task) -> int:
        for i, r in enumerate(self.reads):
            if r is t.read:
                break
        else:
            i = len(self.reads)
            self.reads.append(t.read)
        self.tasks.append(t)
        self.read_of.append(i)
        return len(self.tasks) - 1

    def tup(self, k: int, unit=None):
        t = self.tasks[k]
        if unit is None:
            return (self.read_of[k], t.rr, t.unit, t.score)
        rr = list(t.rr)
        rr[3] = len(unit)
        return (self.read_of[k], tuple(rr), unit, t.score[:len(unit)] if len(unit) <= len(t.score) else np.concatenate([t.score, np.full(len(unit) - len(t.score), -1, np.int32)]))

    def groups(self, index_groups):
        return [[self.tup(k) for k in g] for g in index_groups]


_want = {}


def oracle_revise(orc, t: Task, polish: bool = True):
    """Oracle.revise of the task, computed once per process"""
    key = (id(t.read), t.rr, t.unit.tobytes(), t.score.tobytes(), polish)
    if key not in _want:
        _want[key] = (t.read, orc.revise(t.read, t.rr, t.unit, t.score, polish))
    return _want[key][1]


def polished(orc, t: Task) -> Task:
    """the task as mtr_k_polish leaves it to mtr_k_revise_quads: the polished unit, the record with its length, the node frequencies as they were"""
    res = orc.revise(t.read, t.rr, t.unit, t.score, True)
    n = res["polished_len"]
    unit = np.frombuffer(res["rounds"][0]["in_unit"], np.uint8)
    assert len(unit) == n
    score = t.score[:n] if n <= len(t.score) else np.concatenate([t.score, np.full(n - len(t.score), -1, np.int32)])
    return t.with_unit(unit, score, t.tag + " (polished)")


def round_keys(res):
    """the keys under which the per-read path's round memo files the two rounds of a revision (k2_units.hip.inc: round_lookup): round, rep_start, rep_end,
    period, threshold and unit, all as the round meets them"""
    return [(p, w["in_start"], w["in_end"], w["in_len"], w["threshold"], w["in_unit"]) for p, w in enumerate(res["rounds"])]


def outcome(res, p: int, in_len=None) -> str:
    """a round's outcome for the revised unit: unchanged / longer / shorter / other (same length, other bases)"""
    w = res["rounds"][p]
    if w["unchanged"]:
        return "unchanged"
    return "longer" if w["rev_len"] > w["in_len"] else "shorter" if w["rev_len"] < w["in_len"] else "other"


def cols(U: int) -> int:
    return (U + 15) >> 4                                     # DPQ_COLS


def dpqp_block_bytes(C: int, rows: int) -> int:
    return 4 * (((rows + 1) >> 1) * 16 * C + 16)             # DPQP_BLOCK_BYTES (dp_quad.hip.inc)


def sorted_order(tasks):
    """the chain's sorted order of the revisions: columns per lane descending (classes 0..7 = 8..1 columns), rows descending inside a class"""
    return sorted(range(len(tasks)), key=lambda i: (-cols(tasks[i].U), -tasks[i].rows, i))


def interleaved_order(tasks):
    """short beside long: the sorted order cut into eight stretches and dealt one from each in turn, so that any eight neighbours span the whole order -
    6 beside 128 bases, 5 beside 20 copies, and the units that run by themselves (above 128 bases) beside members of a pass share a wavefront's slots"""
    s = sorted_order(tasks)
    per = (len(s) + 7) // 8
    return [s[c * per + r] for r in range(per) for c in range(8) if c * per + r < len(s)]


# ---- what the tests run --------------------------------------------------------------------------------------------------------------------
GRID_SEED = 8           # chosen so that the oracle shows every outcome in quantity among the eligible tasks (tests/test_revise_cases_ref.py)

_sets = {}


def selection(orc):
    """(grid, ends): the tasks of the grid the entry takes (revise_task.h; the oracle alone runs the others: 21 copies, doubled and very short units), and
    the rep_end = L tasks.  Made once per process."""
    if "sel" not in _sets:
        _sets["sel"] = ([t for t in grid(orc, GRID_SEED) + grid(orc, GRID_SEED + 100, MORE_UNITS, (5, 12)) if eligible(t)], [t for t in end_tasks(orc) if eligible(t)])
    return _sets["sel"]


def by_read(tasks):
    """index groups: the tasks that share a read, in order - the only groups a round memo may see (it is a range's, and a range lies in one read)"""
    out, at = [], {}
    for i, t in enumerate(tasks):
        if id(t.read) not in at:
            at[id(t.read)] = len(out)
            out.append([])
        out[at[id(t.read)]].append(i)
    return out


def single_wave_subset(tasks, step: int = 4):
    """every `step`-th task of the chain's sorted order: a list short enough for one wavefront that still holds every unit length"""
    return [tasks[i] for i in sorted_order(tasks)[::step]]


def memo_groups(orc):
    """groups for the round memo of the per-read path (key: round, rep_start, rep_end, period, threshold, unit; 16 entries), each a list of tasks on one read:
      hit        a task twice
      accept     a task, then the same with mat + 100: equal keys, the same candidate, a higher ratio to beat - acceptance differs
      threshold  a task, then the same with more mismatches claimed: min_missing moves to another digit and round 0 makes another unit
      full       10 tasks whose 20 rounds have 20 distinct keys, then the first and the last again: 16 entries - the first is remembered, the last is not
    Every repeated task changes its unit in round 0, so a round_lookup hit is not also counted as an unchanged unit."""
    if "memo" in _sets:
        return _sets["memo"]
    tasks, _ = selection(orc)
    res = [oracle_revise(orc, t) for t in tasks]
    out = {}
    for t, r in zip(tasks, res):
        w0, w1 = r["rounds"]
        if w0["unchanged"] or not w0["candidate"]:
            continue
        if "hit" not in out and w0["accepted"] and w1["accepted"] and t.U <= 128:
            out["hit"] = [t, t]
        if "accept" not in out and w0["accepted"] and t.U > 128:
            t2 = t.with_rr("claims mat + 100", mat=t.rr[5] + 100)
            r2 = oracle_revise(orc, t2)
            if r2["rounds"][0]["threshold"] == w0["threshold"] and not r2["rounds"][0]["accepted"] and r2["rounds"][0]["rev_unit"] == w0["rev_unit"]:
                out["accept"] = [t, t2]
        if "threshold" not in out and w0["rev_len"] > w0["in_len"]:
            for d in range(1, 200):
                t3 = t.with_rr(f"claims mis + {d}", mis=t.rr[6] + d)
                r3 = oracle_revise(orc, t3)
                if r3["rounds"][0]["threshold"] != w0["threshold"] and r3["rounds"][0]["rev_unit"] != w0["rev_unit"]:
                    out["threshold"] = [t, t3]
                    break
    rng = np.random.RandomState(9)
    c = dc.make_case(rng, 33, 33 * 12 + 3, 7, "noisy", tail=2, tag="memo full")
    full, seen = [], set()
    while len(full) < 10:
        unit = corrupt(rng, c.unit, "sub")
        rr = record(orc, c.read, c.qs, c.qe, unit, 5)
        if rr is None:
            continue
        # (a record that claims 100 matches more: no round is accepted, so round 1 starts from the task's own unit and the ten tasks' twenty keys differ)
        t = Task(c.read, rr, unit, plain_scores(rng, len(unit)), "memo full", 33, 12, "noisy", "sub").with_rr("memo full", mat=rr[5] + 100)
        keys = set(round_keys(oracle_revise(orc, t)))
        if len(keys) == 2 and not keys & seen and not oracle_revise(orc, t)["rounds"][0]["unchanged"]:
            seen |= keys
            full.append(t)
    out["full"] = full + [full[0], full[-1]]
    _sets["memo"] = out
    return out


def cq0_tasks(orc):
    """(A, B): U = 10 over 200 rows and U = 33 over 166 rows on reads of at most 300 bases (one of exactly 300: the batch's cell budget is k2_max_cells(300) =
    302 x 122 = 36 844).  Each fits a pass of its own (2 x DPQP_BLOCK_BYTES = 12 928 and 32 000); side by side at B's three columns per lane and A's 200 rows
    the block is 38 528 bytes: mtr_k_revise_quads runs both by themselves (Cq == 0).  Units with one substitution, so that the rounds have work."""
    if "cq0" in _sets:
        return _sets["cq0"]
    rng = np.random.RandomState(10)
    out = []
    for U, rows, L in ((10, 200, 300), (33, 166, 180)):
        c = dc.make_case(rng, U, rows, 0, "perfect", tail=L - rows - 1, tag="Cq == 0")
        unit = corrupt(rng, c.unit, "sub")
        rr = record(orc, c.read, c.qs, c.qe, unit, 5)
        out.append(Task(c.read, rr, unit, plain_scores(rng, U), "Cq == 0", U, rows // U, "perfect", "sub"))
    _sets["cq0"] = tuple(out)
    return _sets["cq0"]
