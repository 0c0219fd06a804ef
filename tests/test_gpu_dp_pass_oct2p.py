"""The forward pass with EIGHT two-parameter alignments per wavefront (units of up to 32 bases, eight lanes per DP) against the CPU oracle (-m gpu).

Engine.test_wrap_dp_pass("OCT2P", ...) runs the batch path's own device functions (st_fwd2p_oct = dp_forward2p_g16<C, 8>, dp_traceback<0, 1> with the
eight-lane row stride) on groups of the test's choosing, as tests/test_gpu_dp_passes.py does for the other passes.  Every task and both parameter sets
must equal Oracle.wrap_dp on all eight integers:
  every unit length 1 .. 32 (both sides of each eight-column border; 33 is refused: the first length that must not take this pass),
  rows 1, 2, 111, 112, 113 and 225 (either side of the 112-row chunk of the staged window, and of two chunks),
  a window at the very start of the batch and one ending on its last base,
  groups of 1, 2, 5, 7 and 8 members, of one columns-per-lane class and mixed,
  3 rows beside 220 rows in the two halves of one 16-lane row (the early-ended DP stays silent, its neighbour untouched), both ways round,
  a homopolymer unit of one base on a homopolymer window (ties of the maximum).
"""
import numpy as np
import pytest

import mtr_amd
from tests import dp_pass_cases as dc

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 111, 112, 113, 225)
SIZES = (1, 2, 5, 7, 8)


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


def _cols8(U):
    return (U + 7) >> 3


def _check(batch, index_groups, out, orc):
    bad, t = [], 0
    for gi, g in enumerate(index_groups):
        for member, k in enumerate(g):
            c = batch.cases[k]
            for p, s in enumerate(dc.SETS2):
                want, got = dc.oracle_want(orc, c, s), tuple(int(v) for v in out[t, p])
                if want != got:
                    bad.append(f"OCT2P: group {gi} (U {[batch.cases[j].U for j in g]}, rows {[batch.cases[j].rows for j in g]}), member {member}, {c.tag} {c.kind}, "
                               f"U {c.U}, rows {c.rows}, qs {c.qs}, scores {s}: want {want} got {got}")
            t += 1
    assert t == len(out)
    assert not bad, f"{len(bad)} differences, first:\n" + "\n".join(bad[:8])


def _sized_groups(ids, sizes):
    out, at, k = [], 0, 0
    while at < len(ids):
        n = sizes[k % len(sizes)]
        out.append(ids[at:at + n])
        at += n
        k += 1
    return out


def _grid(rng):
    """every unit length 1 .. 32 x every row count; content kind and placement cycle, one case in four ends with its read"""
    out, k = [], 3
    for U in range(1, 33):
        for rows in ROWS:
            kind = dc.KINDS[k % len(dc.KINDS)]
            if kind == "ac" and U & 1:
                kind = "perfect"
            qs = 16 * rng.randint(0, 3) + dc.QS_MOD[(k // len(dc.KINDS)) % 3]
            out.append(dc.make_case(rng, U, rows, qs, kind, (1, 1, 3), rng.randint(0, 4), "grid"))
            k += 1
    return out


def test_oct2p_matches_oracle(eng, orc):
    rng = np.random.RandomState(61)
    b = dc.Batch()
    first, last = dc.placement_cases(np.random.RandomState(77 + 8), 8)        # the batch's first read starts with a window, its last read ends with one
    i_first = b.add(first)
    ids = [b.add(c) for c in _grid(rng)]
    assert len(ids) == 32 * len(ROWS)

    def mk(U, rows, kind="noisy"):
        return b.add(dc.make_case(rng, U, rows, 16 + dc.QS_MOD[(U + rows) % 3], kind, tag="special"))
    groups = [[i_first]]
    for C in range(1, 5):                                    # groups of one columns-per-lane class, as the bins of the batch path make them
        mine = [k for k in ids if _cols8(b.cases[k].U) == C]
        assert len(mine) == 8 * len(ROWS)
        groups += _sized_groups(mine, SIZES)
    mixed = [ids[i] for i in np.random.RandomState(62).permutation(len(ids))]       # and of whatever comes: the pass runs at the longest unit's width
    groups += _sized_groups(mixed, (8, 7, 5, 2, 1))
    # 3 rows beside 220 rows, the two in ONE 16-lane row (members 0 and 1, 2 and 3), both ways round, at every width; the short one's best cell must not
    # move after its last row, and the long one must not see anything of it
    for (ua, ub) in ((5, 7), (16, 9), (17, 24), (32, 25), (3, 32)):
        groups.append([mk(ua, 3, "perfect"), mk(ub, 220, "perfect")])
        groups.append([mk(ub, 220), mk(ua, 3), mk(ua, 220, "perfect"), mk(ub, 3, "two_runs")])
    # ties of the maximum: a one-base unit on a homopolymer window, alone, beside itself and beside others
    h40, h113, h225 = mk(1, 40, "homopolymer"), mk(1, 113, "homopolymer"), mk(1, 225, "homopolymer")
    groups += [[h40], [h113, h113], [h225, mk(2, 30, "ac"), h40, mk(8, 64, "homopolymer"), h113], [mk(32, 33, "homopolymer"), h225]]
    # a full pass of eight around the placements
    groups.append([i_first] + [mk(U, 50 + U) for U in (1, 2, 8, 9, 16, 17)] + [b.add(last)])
    groups.append([b.add(last)])
    assert b.cases[0].qs == 0 and b.read_of[0] == 0 and b.reads[-1] is last.read and last.qe + 1 == len(last.read) - 1
    assert {len(g) for g in groups} >= set(SIZES)
    eng.upload(b.reads)
    out = eng.test_wrap_dp_pass("OCT2P", b.groups(groups))
    _check(b, groups, out, orc)
    assert len(out) > 400


def test_oct2p_refuses_what_the_batch_path_would_not_hand_it(eng, orc):
    rng = np.random.RandomState(63)
    b = dc.Batch()
    ok = b.add(dc.make_case(rng, 32, 40, 1, "noisy"))
    u33 = b.add(dc.make_case(rng, 33, 40, 1, "noisy"))
    long2 = b.add(dc.limit_case(2, dc.dpq_max_rows(2, 1, 3) + 1, (1, 1, 3)))          # one row more than DPQ_FITS(rows, 2, 1, 3) admits
    eng.upload(b.reads)
    for groups, where in (([[ok], [ok, u33]], "task 2"), ([[ok] * 9], "group 0"), ([[long2]], "task 0"), ([[ok], []], "group 1")):
        with pytest.raises(mtr_amd.MtrError, match=f"MTR_ERR_BAD_ARG: bad DP pass .*{where}\\b"):
            eng.test_wrap_dp_pass("OCT2P", b.groups(groups))
    out = eng.test_wrap_dp_pass("OCT2P", b.groups([[ok] * 8]))               # the same task, eligible: it runs, eight times over
    _check(b, [[ok] * 8], out, orc)
