"""Every forward pass of the wrap-around DP against the CPU oracle, on windows, units and groups of the test's choosing (-m gpu).

In a batch run the unit search decides what the passes see.  Here Engine.test_wrap_dp_pass runs ONE pass - the batch path's own device functions -
on the cases of tests/dp_pass_cases.py (tests/test_dp_pass_cases_ref.py shows that they are not degenerate): every unit length either side of a
columns-per-lane border, row counts either side of the staged chunks, windows at both ends of the batch, ties of the maximum, groups of every size with
members of very different lengths, and the last row count each 16-bit pass admits on a perfect repeat.  Every task and parameter set must equal
Oracle.wrap_dp on all eight integers.
"""
import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import dp_pass_cases as dc

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


def _cols(U):
    return (U + 15) >> 4                                   # DPQ_COLS


def _check(name, batch, index_groups, out, orc, two_param):
    """out: [tasks in group order, 2, 8] of the pass `name`"""
    bad, t = [], 0
    for gi, g in enumerate(index_groups):
        for member, k in enumerate(g):
            c = batch.cases[k]
            sets = dc.SETS2 if two_param else ((c.G, c.MM, c.D),)
            for p, s in enumerate(sets):
                want, got = dc.oracle_want(orc, c, s), tuple(int(v) for v in out[t, p])
                if want != got:
                    bad.append(f"{name}: group {gi} {[batch.cases[j].rows for j in g]} rows, member {member}, {c.tag} {c.kind}, U {c.U}, rows {c.rows}, qs {c.qs}, "
                               f"scores {s}: want {want} got {got}")
            if not two_param and out[t, 1].any():
                bad.append(f"{name}: group {gi} member {member}: the second parameter set of a one-parameter pass is not zero: {out[t, 1]}")
            t += 1
    assert t == len(out)
    assert not bad, f"{len(bad)} differences, first:\n" + "\n".join(bad[:8])


def _run(eng, orc, name, batch, index_groups, two_param):
    out = eng.test_wrap_dp_pass(name, batch.groups(index_groups))
    _check(name, batch, index_groups, out, orc, two_param)
    return len(out)


def _sized_groups(ids, sizes):
    """ids cut into groups whose sizes cycle through `sizes`"""
    out, at, k = [], 0, 0
    while at < len(ids):
        n = sizes[k % len(sizes)]
        out.append(ids[at:at + n])
        at += n
        k += 1
    return out


def _upload(eng, batch, last):
    """the batch goes up with the placement cases at its ends: the last read ends on the last row of `last`"""
    assert batch.cases[0].qs == 0 and batch.read_of[0] == 0
    assert batch.reads[-1] is last.read and last.qe + 1 == len(last.read) - 1
    eng.upload(batch.reads)


def _with_placements(batch, cases, U):
    """the cases in a batch whose first read starts with a window and whose last read ends with one"""
    first, last = dc.placement_cases(np.random.RandomState(77 + U), U)
    ids = [batch.add(first)] + [batch.add(c) for c in cases]
    return ids, last


# ---- one alignment per wavefront, both parameter sets ------------------------------------------------------------------------------------
def _wave2p(eng, orc, limits):
    b = dc.Batch()
    ids, last = _with_placements(b, dc.grid(dc.U64, seed=11), 129)
    if limits:
        ids += [b.add(c) for c in dc.wave2p_limits()]
    ids.append(b.add(last))
    _upload(eng, b, last)
    return _run(eng, orc, "WAVE2P", b, [[k] for k in ids], True)


def test_wave2p_matches_oracle(eng, orc):
    """dp_forward2p<1>, dp_forward2p_2c, one DP on 64 lanes (129 .. 256), dp_wrap twice above that; rows 64 000 (packed) and 64 001 (32-bit: dp_forward2<1,2>,
    dp_forward<4>) on perfect repeats; one row more than the four-per-wavefront pass takes"""
    assert _wave2p(eng, orc, True) > 200


def test_wave2p_32_bit_passes_match_oracle(eng, orc, monkeypatch):
    monkeypatch.setenv("MTR_DP16_MAX_ROWS", "0")
    assert _wave2p(eng, orc, False) > 200


# ---- up to four units <= 16 over one window -------------------------------------------------------------------------------------------------
def test_q4_matches_oracle(eng, orc):
    rng = np.random.RandomState(21)
    b = dc.Batch()
    shapes = [(2,), (2, 3, 16), (16, 16, 16, 16), (16,), (15, 16), (1, 2, 16), (3, 16, 5, 2), (16, 2), (7, 7, 7), (16, 1, 16, 1)]
    first, last = dc.placement_cases(np.random.RandomState(77 + 16), 16)      # the batch's first read starts with a window, its last read ends with one

    def over(lead, us, n, kind):
        """the group of `lead` and further units over its window: the lead's unit cut or repeated, or random"""
        g = [b.add(lead)]
        for U in us:
            m = np.resize(lead.unit, U) if n & 1 else rng.randint(0, 4, size=U).astype(np.uint8)
            g.append(b.add(dc.Case(lead.read, lead.qs, lead.qe, m, kind=kind, tag=lead.tag or "q4")))
        return g
    groups, n = [over(first, (2, 16, 9), 1, "noisy")], 0
    for rows in (1, 2, 15, 16, 17, 239, 240, 241, 1007, 1008, 1009):
        for mod in dc.QS_MOD:
            us = shapes[n % len(shapes)]
            kind = dc.KINDS[n % len(dc.KINDS)]
            n += 1
            lead = dc.make_case(rng, us[0], rows, mod, "perfect" if kind == "ac" and us[0] & 1 else kind, tail=n % 3, tag="q4")
            groups.append(over(lead, us[1:], n, kind))
    groups += [over(last, (16, 3, 2), 0, "noisy"), over(last, (), 0, "noisy")]
    _upload(eng, b, last)
    assert _run(eng, orc, "Q4", b, groups, True) > 60


# ---- four alignments per wavefront ------------------------------------------------------------------------------------------------------------
def _special_quads(b, rng, params):
    """groups whose members differ as much as a pass allows: 1 row beside 2 000, (240, 241, 1, 16) rows, 17 beside 32 bases; members of one DPQ_COLS class"""
    def mk(U, rows, kind="noisy", p=0):
        return b.add(dc.make_case(rng, U, rows, 16 + dc.QS_MOD[(U + rows) % 3], kind, params[p % len(params)], tag="special"))
    return [[mk(17, 1), mk(20, 2000, p=1)],
            [mk(32, 2000, "perfect"), mk(17, 1, "perfect", p=2)],
            [mk(100, 240), mk(97, 241, p=1), mk(110, 1, p=2), mk(112, 16)],
            [mk(17, 32, "two_runs"), mk(32, 17, "random", p=1)],
            [mk(5, 241), mk(16, 240, "ac", p=1), mk(2, 16, "homopolymer", p=2), mk(9, 1)]]


def test_quad2p_matches_oracle(eng, orc):
    rng = np.random.RandomState(31)
    b = dc.Batch()
    ids, last = _with_placements(b, dc.grid(dc.U16, seed=12), 33)
    special = _special_quads(b, rng, [(1, 1, 3)])
    limits = []
    for c in dc.quad2p_limits():                             # the last row count DPQ_FITS admits, beside a 1-row alignment and by itself
        limits += [[b.add(dc.make_case(rng, c.U, 1, 3, "perfect", tag="1 row")), b.add(c)], [b.add(c)]]
    ids.append(b.add(last))
    _upload(eng, b, last)
    total = 0
    for C in range(1, 9):                                    # a call takes one columns-per-lane class, as a bin of the batch path
        mine = [k for k in ids if _cols(b.cases[k].U) == C]
        groups = _sized_groups(mine, (1, 2, 3, 4, 4, 3))
        groups += [g for g in special + limits if _cols(b.cases[g[0]].U) == C]
        assert groups
        total += _run(eng, orc, "QUAD2P", b, groups, True)
    assert total > 150


# ---- four and eight revision DPs per wavefront, each with its own parameter set -------------------------------------------------------------------
def _one_param(eng, orc, name, width):
    rng = np.random.RandomState(41 + width)
    b = dc.Batch()
    cases = [c.with_params(dc.SETS3[i % 3]) for i, c in enumerate(dc.grid(dc.U16, seed=13 + width))]
    ids, last = _with_placements(b, cases, 49)
    groups = _sized_groups(ids, tuple(range(1, width + 1)) + (width, 2))
    groups += _special_quads(b, rng, dc.SETS3)
    groups.append([b.add(dc.make_case(rng, 2, 40, 1, "noisy", (5, 1, 1))), b.add(dc.make_case(rng, 128, 300, 15, "noisy", (1, 1, 3)))])      # runs at width 8
    for c in dc.one_param_limits():
        short = dc.make_case(rng, 11, 37, 2, "noisy", dc.SETS3[c.U % 3], tag="short beside a limit")
        groups.append([b.add(c), b.add(short)])              # OCT1P: the limit DP in the low half, the short one in the high half of lane group 0
        groups.append([b.add(short), b.add(c)])              #        and the other way round
        groups.append([b.add(c)])
    groups.append([b.add(last)])
    _upload(eng, b, last)
    return _run(eng, orc, name, b, groups, False)


def test_four1p_matches_oracle(eng, orc):
    assert _one_param(eng, orc, "FOUR1P", 4) > 200


def test_oct1p_matches_oracle(eng, orc):
    assert _one_param(eng, orc, "OCT1P", 8) > 200


# ---- the existing entry: one DP per wavefront, one parameter set -------------------------------------------------------------------------------
def _entry(eng, orc, limits):
    b = dc.Batch()
    cases = [c.with_params(dc.SETS3[i % 3]) for i, c in enumerate(dc.grid(dc.U64, seed=14))]
    ids, last = _with_placements(b, cases, 65)
    if limits:
        ids += [b.add(c) for c in dc.entry_limits()]
    ids.append(b.add(last))
    _upload(eng, b, last)
    out = eng.test_wrap_dp([b.task(k) for k in ids])
    out2 = np.zeros((len(ids), 2, 8), np.int32)
    out2[:, 0] = out
    _check("mtr_test_wrap_dp", b, [[k] for k in ids], out2, orc, False)
    return len(ids)


def test_wrap_dp_entry_matches_oracle(eng, orc):
    """dp_forward<1,2,4,8>, dp_forward_2c and the 64-lane one-parameter pass: the grid, then the largest rows under DP2C_FITS / DPQ_FITS_SC(1, ...) and one
    row more (which takes the 32-bit pass) with each of the three parameter sets"""
    assert _entry(eng, orc, True) > 200


def test_wrap_dp_entry_32_bit_passes_match_oracle(eng, orc, monkeypatch):
    monkeypatch.setenv("MTR_DP16_MAX_ROWS", "0")
    assert _entry(eng, orc, False) > 200


# ---- what the entry refuses, and what it leaves behind ------------------------------------------------------------------------------------------
def test_ineligible_tasks_are_refused_and_the_context_stays_intact(eng, orc):
    rng = np.random.RandomState(51)
    reads = [c for _, c in synth.make_reads("c2", 6, 5)] + [np.tile(np.array([3, 3, 0, 2, 2, 2], np.uint8), 80)]
    want = [orc.process(r) for r in reads]
    assert sum(len(w) for w in want) > 0
    assert [[tuple(r) for r in g] for g in eng.process(reads)] == want

    b = dc.Batch()
    ok = b.add(dc.make_case(rng, 16, 40, 1, "noisy"))
    u17 = b.add(dc.make_case(rng, 17, 40, 1, "noisy"))
    u129 = b.add(dc.make_case(rng, 129, 40, 1, "noisy"))
    long51 = b.add(dc.make_case(rng, 2, 3300, 1, "perfect", (5, 1, 1)))          # 4 (3300 x 5 + 1 x 4) >= 65000
    odd_set = b.add(dc.make_case(rng, 16, 40, 1, "noisy", (2, 1, 1)))
    other_window = b.add(dc.make_case(rng, 5, 40, 1, "noisy"))
    c = b.cases[ok]
    outside = b.add(dc.Case(c.read, c.qs, len(c.read), c.unit))                   # qe = L
    eng.upload(b.reads)
    refused = [("QUAD2P", [[u129]], "task 0"), ("QUAD2P", [[ok], [ok, u17]], "task 2"), ("QUAD2P", [[ok], []], "group 1"), ("QUAD2P", [[ok, ok, ok, ok, ok]], "group 0"),
               ("Q4", [[ok, u17]], "task 1"), ("Q4", [[ok, other_window]], "task 1"), ("WAVE2P", [[ok, ok]], "group 0"), ("WAVE2P", [[ok], [outside]], "task 1"),
               ("FOUR1P", [[ok, long51]], "task 1"), ("OCT1P", [[ok], [ok, odd_set]], "task 2"), ("FOUR1P", [[ok, ok, ok, ok, ok]], "group 0"), ("OCT1P", [[u129]], "task 0")]
    for name, groups, where in refused:
        with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: bad DP pass .*{where}\\b"):
            eng.test_wrap_dp_pass(name, b.groups(groups))
    for name, two in (("QUAD2P", True), ("OCT1P", False), ("WAVE2P", True)):     # the same tasks, eligible: they run
        _run(eng, orc, name, b, [[ok]], two)
    assert [[tuple(r) for r in g] for g in eng.process(reads)] == want
