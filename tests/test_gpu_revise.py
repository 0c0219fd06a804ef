"""The revision rounds against the CPU oracle on records and units of the test's choosing (-m gpu).

In a batch run the unit search decides which records, units and neighbours a revision meets.  Here Engine.test_revise hands the tasks of
tests/revise_cases.py (tests/test_revise_cases_ref.py shows from the oracle alone that every outcome of a round occurs among them) to the two
places revisions run:
  WAVE   revise() - polish_repeat, the two rounds, the per-read path's round memo - a group of tasks after the other on one wavefront
  SLOTS  mtr_k_revise_quads ITSELF on a work list in the test's order: the eight-slot machine, its passes of 1 .. 8 members, the by-itself DPs
Every task's 13 record fields and unit bytes must equal Oracle.revise exactly.  docs/revision_tests.md says what each set is for.
"""
import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import revise_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    from tests.oracle_binding import Oracle
    o = Oracle()
    yield o
    o.close()


def _batch(tasks, last=()):
    """the tasks' reads in the order first used, those of `last` behind them: the batch's last read then ends on a record's last row"""
    b = rc.Tasks()
    ids = [b.add(t) for t in list(tasks) + list(last)]
    return b, ids


def _run(eng, orc, mode, b, index_groups, waves=0, prepared=False):
    """the groups through the entry, every task against the oracle; SLOTS takes the polished unit (prepared: the tasks are polished already)"""
    slots = mode == "SLOTS"
    if slots and not prepared:
        sent = {k: rc.polished(orc, b.tasks[k]) for g in index_groups for k in g}
        groups = [[(b.read_of[k], sent[k].rr, sent[k].unit, sent[k].score) for k in g] for g in index_groups]
    else:
        sent = {k: b.tasks[k] for g in index_groups for k in g}
        groups = b.groups(index_groups)
    got, cells = eng.test_revise(mode, groups, waves=waves)
    bad, at = [], 0
    for gi, g in enumerate(index_groups):
        for pos, k in enumerate(g):
            want = rc.oracle_revise(orc, sent[k], not slots)
            rr, unit = got[at]
            if rr != want["rr"] or unit.tobytes() != want["unit"].tobytes():
                bad.append(f"{mode} waves={waves}: task {at} (group {gi}, position {pos} of {len(g)}) {sent[k]!r}:\n    want {want['rr']} unit {want['unit'].tolist()[:40]}"
                           f"\n    got  {rr} unit {unit.tolist()[:40]}")
            at += 1
    assert at == len(got)
    assert not bad, f"{len(bad)} of {at} tasks differ, first:\n" + "\n".join(bad[:6])
    if not slots:
        c, (dps, hits) = eng.counters(), _memo_model(orc, b, index_groups)
        print(f"WAVE, {len(index_groups)} groups, {at} tasks: revise_dp_calls {c['revise_dp_calls']} (model {dps}), memo_hits {c['memo_hits']} (model {hits})")
        assert (c["revise_dp_calls"], c["memo_hits"]) == (dps, hits)
    return at, cells


def _memo_model(orc, b, index_groups):
    """what the round memo of revise() must do for these groups, from the oracle's rounds alone: a round whose key (round, rep_start, rep_end, period,
    threshold, unit - all as the round meets them) lies in the group's memo is answered from it; any other runs its vote DP, takes entry rmemo_n while there
    are fewer than 16, and - if its votes leave the unit as it was - takes the vote DP's result for the re-alignment, which counts as a hit too.
    -> (vote DPs run, memo_hits)"""
    dps = hits = 0
    for g in index_groups:
        memo = set()
        for k in g:
            res = rc.oracle_revise(orc, b.tasks[k], True)
            for key, w in zip(rc.round_keys(res), res["rounds"]):
                if key in memo:
                    hits += 1
                    continue
                if len(memo) < 16:
                    memo.add(key)
                dps += 1
                hits += w["unchanged"]
    return dps, hits


def _oracle_rounds(orc, b, index_groups, polish=True):
    """(rounds the oracle ran, rounds whose votes left the unit as it was) for the groups' tasks"""
    res = [rc.oracle_revise(orc, b.tasks[k], polish) for g in index_groups for k in g]
    return 2 * len(res), sum(w["unchanged"] for r in res for w in r["rounds"])


# ---- WAVE: revise() ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_batch(eng, orc):
    tasks, ends = rc.selection(orc)
    b, ids = _batch(tasks, ends)
    assert b.tasks[ids[0]].rr[0] <= 1 and b.read_of[ids[0]] == 0
    assert b.reads[-1] is ends[-1].read and ends[-1].rr[1] == len(ends[-1].read)
    return b, ids


def test_wave_grid_matches_oracle(eng, orc, grid_batch):
    """the grid and the rep_end = L records, the tasks of a read (the corruptions of its unit) as one group"""
    b, ids = grid_batch
    eng.upload(b.reads)
    n, _ = _run(eng, orc, "WAVE", b, rc.by_read(b.tasks))
    assert n == len(ids) > 700
    c = eng.counters()
    assert c["revise_dp_calls"] > 0 and c["memo_hits"] > 0


def test_wave_results_do_not_depend_on_the_groups(eng, orc, grid_batch):
    """the same tasks as singleton groups, and the tasks of a read shuffled and cut into groups of other sizes: what the memo holds when a task arrives differs,
    its result must not"""
    b, ids = grid_batch
    eng.upload(b.reads)
    _run(eng, orc, "WAVE", b, [[k] for k in ids])
    rng = np.random.RandomState(12)
    groups = []
    for g in rc.by_read(b.tasks):
        g = [g[i] for i in rng.permutation(len(g))] + [g[0]]
        cut = 1 + rng.randint(0, len(g))
        groups += [g[:cut]] + ([g[cut:]] if g[cut:] else [])
    _run(eng, orc, "WAVE", b, groups, waves=7)


def test_wave_polish_slice(eng, orc):
    tasks = [t for t in rc.polish_tasks(orc) if rc.eligible(t)]
    b, ids = _batch(tasks)
    eng.upload(b.reads)
    n, _ = _run(eng, orc, "WAVE", b, rc.by_read(b.tasks))
    assert n == len(tasks) > 100


def test_wave_memo_groups(eng, orc):
    """the memo's key and capacity: a hit, a hit whose acceptance differs, a miss on the threshold alone, and a group that overflows the 16 entries.  The vote
    DPs run are fewer than the rounds the oracle ran; memo_hits (round_lookup hits + rounds whose votes left the unit unchanged, which take the vote DP's
    result) exceeds the oracle's unchanged rounds, so look-ups did hit."""
    m = rc.memo_groups(orc)
    names = ("hit", "accept", "threshold", "full")
    b, _ = _batch([t for n in names for t in m[n]])
    groups, at = [], 0
    for n in names:
        groups.append(list(range(at, at + len(m[n]))))
        at += len(m[n])
    eng.upload(b.reads)
    _run(eng, orc, "WAVE", b, groups)
    c = eng.counters()
    rounds, unchanged = _oracle_rounds(orc, b, groups)
    print(f"memo groups: oracle rounds {rounds}, unchanged {unchanged}; revise_dp_calls {c['revise_dp_calls']}, memo_hits {c['memo_hits']}")
    assert c["revise_dp_calls"] < rounds
    assert c["memo_hits"] > unchanged
    # each group alone (_run holds both counters to the model of the memo each time)
    for g, n in zip(groups, names):
        _run(eng, orc, "WAVE", b, [g])
        c = eng.counters()
        rounds, unchanged = _oracle_rounds(orc, b, [g])
        if n == "threshold":
            assert c["revise_dp_calls"] == rounds            # equal but for the threshold: no hit
        else:
            assert c["revise_dp_calls"] < rounds, n
        if n == "full":
            assert c["revise_dp_calls"] == rounds - 2          # the first task again: two hits; the last again: none, its rounds found the memo full


# ---- SLOTS: mtr_k_revise_quads itself ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_wave(orc):
    """the list one wavefront takes: every fourth task of the grid's sorted order, the rep_end = L records' reads last"""
    tasks, ends = rc.selection(orc)
    sub = rc.single_wave_subset(tasks)
    b, ids = _batch(sub, ends)
    return b, ids, len(sub)


def test_slots_singleton_lists(eng, orc, one_wave):
    """a list of ONE revision per launch: every pass has one member (matrix 0 of its block) or the DP runs by itself - each width of a pass, a by-itself unit,
    and the records that end on L"""
    b, ids, n_sub = one_wave
    eng.upload(b.reads)
    seen, picked = set(), []
    for k in rc.sorted_order(b.tasks[:n_sub]):
        c = min(rc.cols(b.tasks[k].U), 9)
        if c not in seen:
            seen.add(c)
            picked.append(ids[k])
    assert len(picked) == 9
    for k in picked + ids[n_sub:]:
        _run(eng, orc, "SLOTS", b, [[k]], waves=1)


def test_slots_list_lengths(eng, orc, one_wave):
    """lists of 2, 4, 5, 8, 9 and 17 revisions on one wavefront: passes of 1 .. 8 members, and the list runs out with slots still busy"""
    b, ids, n_sub = one_wave
    eng.upload(b.reads)
    order = [ids[k] for k in rc.interleaved_order(b.tasks[:n_sub])]
    at = 0
    for n in (2, 4, 5, 8, 9, 17):
        _run(eng, orc, "SLOTS", b, [order[at:at + n]], waves=1)
        at += n
    _run(eng, orc, "SLOTS", b, [ids[n_sub:]], waves=1)                  # the records that end on L, side by side


def test_slots_sorted_list(eng, orc, one_wave):
    """the chain's order (columns per lane, rows): neighbours of like width share the passes"""
    b, ids, n_sub = one_wave
    eng.upload(b.reads)
    order = [ids[k] for k in rc.sorted_order(b.tasks[:n_sub])] + ids[n_sub:]
    n, _ = _run(eng, orc, "SLOTS", b, [order], waves=1)
    assert 100 < n <= 210
    assert eng.counters()["qpass_cells_rev"] > 0


@pytest.mark.parametrize("dp16", [None, "100", "0"])
def test_slots_interleaved_list(eng, orc, one_wave, monkeypatch, dp16):
    """6 beside 128 bases, 5 beside 20 copies, by-itself units beside members of a pass in one wavefront's slots; MTR_DP16_MAX_ROWS=100: the windows of more
    than 100 rows run by themselves beside the others' passes; 0: every DP by itself - no pass, the same records"""
    b, ids, n_sub = one_wave
    if dp16 is not None:
        monkeypatch.setenv("MTR_DP16_MAX_ROWS", dp16)
    eng.upload(b.reads)
    order = [ids[k] for k in rc.interleaved_order(b.tasks[:n_sub])] + ids[n_sub:]
    _run(eng, orc, "SLOTS", b, [order], waves=1)
    cells = eng.counters()["qpass_cells_rev"]
    if dp16 == "0":
        assert cells == 0
    else:
        assert cells > 0
    test_slots_interleaved_list.cells[dp16] = cells
    if dp16 == "100" and None in test_slots_interleaved_list.cells:
        assert cells < test_slots_interleaved_list.cells[None]          # fewer cells went through passes


test_slots_interleaved_list.cells = {}


@pytest.mark.parametrize("waves", [4, 64])
def test_slots_whole_grid(eng, orc, grid_batch, waves):
    b, ids = grid_batch
    eng.upload(b.reads)
    order = [ids[k] for k in rc.interleaved_order(b.tasks)] if waves == 4 else [ids[k] for k in rc.sorted_order(b.tasks)]
    n, _ = _run(eng, orc, "SLOTS", b, [order], waves=waves)
    assert 700 < n <= 1000
    assert eng.counters()["qpass_cells_rev"] > 0


def test_slots_members_fit_alone_but_not_side_by_side(eng, orc):
    """Cq == 0: with reads of at most 300 bases the cell budget is 36 844; A (10 bases, 200 rows) and B (33 bases, 166 rows) each fit a pass of their own, side by
    side at three columns per lane and 200 rows they do not - both run by themselves, so the pair sends fewer cells through passes than the two alone"""
    a, bb = rc.cq0_tasks(orc)
    b, ids = _batch([a, bb])
    eng.upload(b.reads)
    cells_rev = {}
    for name, lst in (("A", [ids[0]]), ("B", [ids[1]]), ("AB", ids)):
        _, budget = _run(eng, orc, "SLOTS", b, [lst], waves=1)
        cells_rev[name] = eng.counters()["qpass_cells_rev"]
    print(f"Cq == 0: budget {budget}, qpass_cells_rev {cells_rev}")
    assert 2 * rc.dpqp_block_bytes(rc.cols(a.U), a.rows) == 12928 <= budget
    assert 2 * rc.dpqp_block_bytes(rc.cols(bb.U), bb.rows) == 32000 <= budget
    assert 2 * rc.dpqp_block_bytes(max(rc.cols(a.U), rc.cols(bb.U)), max(a.rows, bb.rows)) == 38528 > budget
    assert cells_rev["A"] > 0 and cells_rev["B"] > 0
    assert cells_rev["AB"] < cells_rev["A"] + cells_rev["B"]


# ---- what the entry refuses, and what it leaves behind -----------------------------------------------------------------------------------------
def _refusal_batch(orc):
    tasks, _ = rc.selection(orc)
    ok = next(t for t in tasks if t.U == 17 and t.how == "exact" and t.copies == 12)
    other = next(t for t in tasks if t.U == 33 and t.how == "exact" and t.copies == 12)
    b, ids = _batch([ok, other])
    return b, ok, ids


REFUSALS = {
    "period below 6": (lambda t: t.with_unit(t.unit[:5], t.score[:5], ""), "period outside 6..499"),
    "period above 499": (lambda t: t.with_unit(np.resize(t.unit, 500), np.resize(t.score, 500), "").with_rr("", repeat_len=5000), "period outside 6..499"),
    "unit of another length": (lambda t: t.with_rr("", period=t.U + 1), "the unit's length is not the period"),
    "coverage below 5": (lambda t: t.with_rr("", repeat_len=4 * t.U + t.U - 1), "coverage outside 5..20"),
    "coverage above 20": (lambda t: t.with_rr("", repeat_len=21 * t.U), "coverage outside 5..20"),
    "rep_start below 0": (lambda t: t.with_rr("", rep_start=-1), "window outside"),
    "rep_end beyond L": (lambda t: t.with_rr("", rep_end=len(t.read) + 1), "window outside"),
    "rep_end before rep_start": (lambda t: t.with_rr("", rep_end=t.rr[0] - 1), "window outside"),
    "no counts": (lambda t: t.with_rr("", mat=0, mis=0, ins=0, del_=0), "non-positive counts"),
    "repeat_len 0": (lambda t: t.with_rr("", repeat_len=0), "non-positive counts"),
    "k below 2": (lambda t: t.with_rr("", k=1), "k outside 2..15"),
    "k above 15": (lambda t: t.with_rr("", k=16), "k outside 2..15"),
    "unit code": (lambda t: t.with_unit(np.where(np.arange(t.U) == 3, 4, t.unit).astype(np.uint8), t.score, ""), "a unit code above 3"),
}


@pytest.mark.parametrize("mode", ["WAVE", "SLOTS"])
@pytest.mark.parametrize("reason", sorted(REFUSALS))
def test_ineligible_tasks_are_refused(eng, orc, mode, reason):
    b, ok, ids = _refusal_batch(orc)
    eng.upload(b.reads)
    make, words = REFUSALS[reason]
    bad = make(ok)
    good = (0, ok.rr, ok.unit, ok.score)
    with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: bad revision task 2 \\(group 1\\): {words}"):
        eng.test_revise(mode, [[good, good], [(0, bad.rr, bad.unit, bad.score)]])


def test_groups_and_lists_are_refused_and_the_context_stays_intact(eng, orc, monkeypatch):
    reads = [c for _, c in synth.make_reads("c2", 6, 5)] + [np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 80)]
    want = [orc.process(r) for r in reads]
    assert sum(len(w) for w in want) > 0
    assert [[tuple(r) for r in g] for g in eng.process(reads)] == want

    b, ok, ids = _refusal_batch(orc)
    eng.upload(b.reads)
    good, other = b.tup(ids[0]), b.tup(ids[1])
    for mode in ("WAVE", "SLOTS"):
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: bad revision task 1 \\(group 1\\): empty group"):
            eng.test_revise(mode, [[good], [], [good]])
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: bad revision task: no group"):
            eng.test_revise(mode, [])
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: bad revision task 4096 \\(group 0\\): more tasks than the lists hold"):
            eng.test_revise(mode, [[good] * 4097])
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: bad revision task 0 \\(group 0\\): read outside the batch"):
            eng.test_revise(mode, [[(2, ok.rr, ok.unit, ok.score)]])
    with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: bad revision task 1 \\(group 0\\): the tasks of a WAVE group share their read"):
        eng.test_revise("WAVE", [[good, other]])
    _run(eng, orc, "SLOTS", b, [[ids[0], ids[1]]])             # a list may: the slots of a wavefront hold revisions of any reads
    _run(eng, orc, "WAVE", b, [[ids[0]], [ids[1]]])            # the same tasks, eligible: they run
    # beyond WrapDPsize: a context made under a lowered limit refuses what the rounds could not align ((2 x 17 + 1) rows + 34 >= the limit)
    monkeypatch.setenv("MTR_TEST_WRAP_DP_SIZE", str(35 * ok.rows + 34))
    e2 = mtr_amd.Engine()
    try:
        e2.upload(b.reads)
        for mode in ("WAVE", "SLOTS"):
            with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: bad revision task 0 \\(group 0\\): period x rows beyond WrapDPsize"):
                e2.test_revise(mode, [[good]])
        fresh = mtr_amd.Engine()
        try:
            with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: bad revision task: no batch uploaded"):
                fresh.test_revise("WAVE", [[good]])
        finally:
            fresh.close()
    finally:
        e2.close()
        monkeypatch.delenv("MTR_TEST_WRAP_DP_SIZE")
        mtr_amd.Engine().close()                               # the device's limit back to the built-in one
    assert [[tuple(r) for r in g] for g in eng.process(reads)] == want
