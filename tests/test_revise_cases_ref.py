"""The revision's cases (tests/revise_cases.py) and the oracle's export of the revision alone (mtro_revise), on the CPU.

The export must be the oracle's own revision: Oracle.process on reads with revisions gives what it gave before the export existed (the pinned golden
records), and what the export reports per round equals the G3r capture lines mtro_process_read leaves for the same record.  The cases must not be
degenerate: every claim below is asserted FROM THE ORACLE ALONE on the very selection tests/test_gpu_revise.py runs - conditions on the inputs, not
tolerances.
"""
import collections
import json

import numpy as np
import pytest

from mtr_amd import synth
from tests import revise_cases as rc


@pytest.fixture(scope="module")
def orc():
    from tests.oracle_binding import Oracle
    o = Oracle()
    yield o
    o.close()


def _reads():
    return [c for _, c in synth.make_reads("c2", 12, 5)] + [np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 80)]


def _capture(orc, reads, path):
    orc.capture(str(path), 1)
    try:
        recs = [orc.process(r) for r in reads]
    finally:
        orc.end_capture()
    per_read, cur = [], None
    for line in open(path):
        e = json.loads(line)
        if e["t"] == "G1":
            cur = []
            per_read.append(cur)
        else:
            cur.append(e)
    return recs, per_read


def test_the_export_is_the_revision_of_process_read(orc, tmp_path):
    """every revision of a few reads: polish's capture line (G3p) gives the record's window, k, unit and node frequencies, the first G3r line behind it
    repeat_len, mis, ins, del (mat = repeat_len - mis - ins: every row of the repeat is a match, a mismatch or an insertion); the export, given that
    record, must report the two G3r lines' fields and units, and leave no line of its own"""
    reads = _reads()
    recs, per_read = _capture(orc, reads, tmp_path / "a.jsonl")
    code = {c: i for i, c in enumerate("ACGT")}
    n_rev = changed = 0
    orc.capture(str(tmp_path / "b.jsonl"), 1)
    try:
        for read, ev in zip(reads, per_read):
            for i, e in enumerate(ev):
                if e["t"] != "G3p":
                    continue
                g = [x for x in ev[i + 1:] if x["t"] in ("G3r", "G3p")][:2]
                assert [x["t"] for x in g] == ["G3r", "G3r"]
                unit = np.array([code[c] for c in e["in"]], np.uint8)
                r0 = g[0]
                mat = r0["repeat_len"] - r0["mis"] - r0["ins"]
                rr = (e["rep_start"], e["rep_end"], r0["repeat_len"], len(unit), (mat + r0["mis"] + r0["del"]) // len(unit), mat, r0["mis"], r0["ins"], r0["del"],
                      e["k"], 1, 1, 3)
                res = orc.revise(read, rr, unit, e["in_score"], True)
                assert res["polished_len"] == len(e["out"])
                for w, x in zip(res["rounds"], g):
                    got = (w["in_start"], w["in_end"], w["in_repeat_len"], w["in_mis"], w["in_ins"], w["in_del"], "".join("ACGT"[b] for b in w["in_unit"]),
                           w["rev_len"], "".join("ACGT"[b] for b in w["rev_unit"]))
                    want = (x["rep_start"], x["rep_end"], x["repeat_len"], x["mis"], x["ins"], x["del"], x["in"], x["out_period"], x["out"])
                    assert got == want
                n_rev += 1
                changed += res["rounds"][0]["unchanged"] == 0
    finally:
        orc.end_capture()
    assert n_rev >= 20 and changed >= 3
    assert open(tmp_path / "b.jsonl").read() == ""          # the export leaves no capture line
    again, per_read2 = _capture(orc, reads, tmp_path / "c.jsonl")
    assert again == recs and per_read2 == per_read           # and leaves the context as it was


def test_process_is_unchanged_on_reads_with_revisions(orc):
    """the golden records of the pinned cases were made before the export: the restated revise() gives them still (tests/test_oracle_golden.py holds every
    capture point; here the reads with revisions, after calls of the export in between)"""
    reads = _reads()
    before = [orc.process(r) for r in reads]
    tasks, _ = rc.selection(orc)
    for t in tasks[:40]:
        rc.oracle_revise(orc, t)
    assert [orc.process(r) for r in reads] == before
    assert sum(len(r) for r in before) > 0


def test_the_export_refuses_what_it_documents(orc):
    tasks, _ = rc.selection(orc)
    t = tasks[0]
    L = len(t.read)

    def refused(code, rr=t.rr, unit=t.unit, score=t.score, read=t.read, o=orc):
        with pytest.raises(ValueError, match=f"\\({code}\\)"):
            o.revise(read, rr, unit, score)

    def rr(**f):
        return t.with_rr("", **f).rr
    refused(-2, rr=rr(period=0), unit=t.unit[:0], score=t.score[:0])
    refused(-2, rr=rr(period=500), unit=np.zeros(500, np.uint8), score=np.zeros(500, np.int32))
    refused(-2, rr=rr(period=t.U + 1))
    refused(-3, rr=rr(rep_start=-1))
    refused(-3, rr=rr(rep_end=L + 1))
    refused(-3, rr=rr(rep_start=t.rr[1] + 1))
    refused(-4, rr=rr(mat=0, mis=0, ins=0, del_=0))
    refused(-4, rr=rr(repeat_len=0))
    refused(-5, rr=rr(k=0))
    refused(-7, unit=np.full(t.U, 4, np.uint8))
    orc.revise(t.read, rr(rep_end=L), t.unit, t.score)      # rep_end = L is taken
    from tests.oracle_binding import Oracle
    fo = Oracle()
    fo.set_file_order(True)
    try:
        refused(-1, o=fo)
    finally:
        fo.close()


def test_every_outcome_of_a_round_occurs_in_quantity(orc):
    tasks, ends = rc.selection(orc)
    assert 600 <= len(tasks) <= 1000 and len(ends) >= 3
    acc, out0, out1 = collections.Counter(), collections.Counter(), collections.Counter()
    inserted = moved = 0
    for t in tasks + ends:
        r = rc.oracle_revise(orc, t)
        assert r["polished_len"] == t.U and r["rounds"][0]["in_unit"] == t.unit.tobytes()               # plain node frequencies: polish changes nothing,
        q = rc.oracle_revise(orc, rc.polished(orc, t), False)                                            # the task serves both modes
        assert (q["rr"], q["unit"].tobytes()) == (r["rr"], r["unit"].tobytes())
        w0, w1 = r["rounds"]
        acc[(w0["accepted"], w1["accepted"])] += 1
        out0[rc.outcome(r, 0)] += 1
        out1[rc.outcome(r, 1)] += 1
        for w in (w0, w1):
            inserted += w["rev_len"] > w["in_len"] and w["threshold"] >= 0
            moved += bool(w["accepted"] and w["moved"])
    for pattern in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert acc[pattern] >= 10, acc
    for o in ("unchanged", "longer", "shorter", "other"):
        assert out0[o] >= 10 and out1[o] >= 5, (out0, out1)
    assert inserted >= 10 and moved >= 10
    assert sum(t.rr[1] == len(t.read) for t in ends) >= 3
    assert ends[0].rr[0] == 0                                # a record that starts on base 0 of its read
    assert tasks[0].read is rc.selection(orc)[0][0].read and min(t.rr[0] for t in tasks if t.read is tasks[0].read) <= 1
    assert sum(len(t.read) == t.rr[1] + 1 or len(t.read) == t.rr[1] + 2 for t in tasks) >= 10           # reads with no base behind the window
    # every unit length of the grid, either side of the borders, both kinds of pass member and the by-itself units
    assert {t.U0 for t in tasks} == set(rc.UNITS + rc.MORE_UNITS)
    assert {rc.cols(t.U) for t in tasks if t.U <= 128} == set(range(1, 9))
    assert sum(t.U > 226 for t in tasks) >= 10 and sum(128 < t.U <= 226 for t in tasks) >= 10
    assert {t.coverage for t in tasks} >= {5, 6, 12, 20}


def test_the_unselected_grid_is_what_the_entry_refuses(orc):
    full = rc.grid(orc, rc.GRID_SEED)
    assert len(full) >= 850
    out = [t for t in full if not rc.eligible(t)]
    assert len(out) >= 200 and all(not 5 <= t.coverage <= 20 or t.U < 6 for t in out)
    for t in out[::10]:
        rc.oracle_revise(orc, t)                             # the oracle runs them all the same


def test_polish_slice(orc):
    tasks = [t for t in rc.polish_tasks(orc) if rc.eligible(t)]
    assert 100 <= len(tasks) <= 300
    changed = differs = 0
    for t in tasks:
        a, b = rc.oracle_revise(orc, t, True), rc.oracle_revise(orc, t, False)
        changed += a["polished_len"] != t.U or a["rounds"][0]["in_unit"] != t.unit.tobytes()
        differs += a["rr"] != b["rr"] or a["unit"].tobytes() != b["unit"].tobytes()
    assert changed >= 10 and differs >= 3, (changed, differs)


def test_memo_groups(orc):
    m = rc.memo_groups(orc)
    assert set(m) == {"hit", "accept", "threshold", "full"}
    for name, g in m.items():
        assert all(t.read is g[0].read for t in g), name
        assert all(rc.eligible(t) for t in g), name
    res = {name: [rc.oracle_revise(orc, t) for t in g] for name, g in m.items()}
    # a repeated task's round 0 changes its unit: its round_lookup hit is not an unchanged unit as well
    for name, k in (("hit", 0), ("full", 0), ("full", 9)):
        assert not res[name][k]["rounds"][0]["unchanged"]
    a, b = m["accept"]
    ra, rb = res["accept"]
    assert a.unit.tobytes() == b.unit.tobytes() and a.rr[:4] == b.rr[:4] and b.rr[5] == a.rr[5] + 100
    assert ra["rounds"][0]["threshold"] == rb["rounds"][0]["threshold"] and ra["rounds"][0]["rev_unit"] == rb["rounds"][0]["rev_unit"]
    assert ra["rounds"][0]["accepted"] == 1 and rb["rounds"][0]["accepted"] == 0
    a, b = m["threshold"]
    ra, rb = res["threshold"]
    assert a.unit.tobytes() == b.unit.tobytes() and a.rr[:4] == b.rr[:4]
    assert ra["rounds"][0]["threshold"] != rb["rounds"][0]["threshold"] and ra["rounds"][0]["rev_unit"] != rb["rounds"][0]["rev_unit"]
    full = m["full"]
    assert len(full) == 12 and len({t.unit.tobytes() for t in full[:10]}) == 10 and full[10] is full[0] and full[11] is full[9]
    keys = [k for r in res["full"][:10] for k in rc.round_keys(r)]
    assert len(set(keys)) == 20 > 16                         # K2_RMEMO_N: the ninth and tenth tasks' rounds find the memo full


def test_cq0_numbers(orc):
    a, b = rc.cq0_tasks(orc)
    assert (a.U, a.rows, b.U, b.rows) == (10, 200, 33, 166) and max(len(a.read), len(b.read)) == 300
    assert rc.eligible(a) and rc.eligible(b)
    cells = 302 * 122                                        # k2_max_cells(300); the GPU test takes the number from the entry
    assert 2 * rc.dpqp_block_bytes(rc.cols(a.U), a.rows) == 12928 <= cells
    assert 2 * rc.dpqp_block_bytes(rc.cols(b.U), b.rows) == 32000 <= cells
    assert 2 * rc.dpqp_block_bytes(3, 200) == 38528 > cells
    for t in (a, b):
        assert not rc.oracle_revise(orc, t, False)["rounds"][0]["unchanged"]


def test_orders(orc):
    tasks, _ = rc.selection(orc)
    s, i = rc.sorted_order(tasks), rc.interleaved_order(tasks)
    assert sorted(s) == sorted(i) == list(range(len(tasks)))
    assert [rc.cols(tasks[k].U) for k in s] == sorted((rc.cols(t.U) for t in tasks), reverse=True)
    sub = rc.single_wave_subset(tasks)
    assert 100 <= len(sub) <= 200 and {t.U0 for t in sub} >= set(rc.UNITS)
    il = [sub[k] for k in rc.interleaved_order(sub)]
    # windows of eight neighbours of the interleaved list: 6 beside 128 bases, 5 beside 20 copies, by-itself units beside members of a pass
    wins = [il[k:k + 8] for k in range(0, len(il) - 7, 8)]       # one wavefront fills its eight slots with the list's first eight, ...
    assert any(min(t.U for t in w) <= 7 and any(113 <= t.U <= 128 for t in w) for w in wins)
    assert any(min(t.coverage for t in w) == 5 and max(t.coverage for t in w) == 20 for w in wins)
    assert any(any(t.U > 128 for t in w) and any(t.U <= 128 for t in w) for w in wins)
    assert any(t.rows > 100 for t in sub) and any(t.rows <= 100 for t in sub)              # MTR_DP16_MAX_ROWS=100 splits the list
