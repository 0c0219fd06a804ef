"""tests/range_cases.py against the CPU oracle and the source: every read is what its claim says (no GPU).

The GPU file tests/test_gpu_ranges_parts.py runs these reads through the three-kernel range finder; here the claims that make them the right
reads are checked - pass and segment counts, which pass records what, which form of phase D a read takes - so that a later change of a
constant fails this file instead of quietly moving the path away from the cases.  `python -m pytest -s` prints the case table.
"""
import os
import re

import numpy as np
import pytest

from tests import range_cases as rc
from tests.oracle_binding import Oracle

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mtr_amd", "csrc")
MODES = (True, False)                      # Manhattan, Pearson


@pytest.fixture(scope="module")
def table():
    """name -> {manhattan: (ranges, raw, di_passes)}: one oracle run per read and DI mode, shared by every test"""
    out = {}
    for m in MODES:
        o = Oracle(m)
        for name, c in rc.cases().items():
            o.lib.mtro_reset_stats(o.h)
            ranges, raw = o.ranges_raw(c.codes)
            out.setdefault(name, {})[m] = (ranges, raw, o.stats()["di_passes"])
        o.close()
    return out


def _surviving_passes(L, ranges, raw):
    """indices, in the read's own pass list, of the passes with a range that survives the de-duplication"""
    k_at = {int(s): int(k) for s, _, _, k in raw}
    mine = rc.passes(L)
    return {mine.index((k_at[s], w)) for s, _, w, _ in ranges}


def test_the_constants_are_the_sources():
    k1 = open(os.path.join(CSRC, "k1_ranges.hip.inc")).read()
    abi = open(os.path.join(CSRC, "mtr_abi.hip")).read()
    ent = open(os.path.join(CSRC, "test_entries.hip.inc")).read()
    common = open(os.path.join(CSRC, "mtr_common.h")).read()
    assert re.search(r"#define K1_TILE %d\b" % rc.TILE, k1) and re.search(r"#define K1_PIPE_WAVES %d\b" % rc.PIPE_WAVES, k1)
    assert re.search(r"#define K1_WIN %d\b" % rc.DEDUP_WINDOW, k1)
    assert "#define K1_PIPE_ARENA_BYTES (K1_PIPE_WAVES * K1_TILE * 16)" in k1 and "(cnt + 1) * 20 <= arena_bytes" in k1
    assert "DEVINL int k1_seg_len(int n) { int s = ((n + 63) / 64 + 63) & ~63; return s < 512 ? 512 : s; }" in k1
    assert "int sl = ((nn + 63) / 64 + 63) & ~63; if (sl < 512) sl = 512;" in abi                  # launch_k1_parts: the host's copy
    assert re.search(r"const long parts_max = %d;" % rc.PARTS_MAX, abi) and re.search(r"const int parts_max = %d;" % rc.PARTS_MAX, ent)
    assert re.search(r"#define MTRC_MIN_WINDOW\s+%d\b" % rc.MIN_WINDOW, common) and re.search(r"#define MTRC_MAX_WINDOW\s+%d\b" % rc.MAX_WINDOW, common)
    assert rc.LDS_LIST_MAX == 6552 and len(rc.ALL_PASSES) == 20


def test_pass_thresholds(table):
    for L in (1, 2, 10):
        assert rc.passes(L) == [] and rc.work_items(L) == 0
    for w in rc.WINDOWS:
        lo, hi = rc.cases()[f"threshold_{2 * w + 1}"], rc.cases()[f"threshold_{2 * w + 2}"]
        assert (lo.L, hi.L) == (2 * w + 1, 2 * w + 2)
        assert (5, w) not in rc.passes(lo.L) and (5, w) in rc.passes(hi.L)
        assert len(rc.passes(hi.L)) > len(rc.passes(lo.L))
    assert len(rc.passes(2561)) == 16 and len(rc.passes(2562)) == 17 and len(rc.passes(20481)) == 19 and len(rc.passes(20482)) == 20
    # the enumeration is the oracle's: it runs exactly these passes on every read, in both modes
    for name, c in rc.cases().items():
        for m in MODES:
            assert table[name][m][2] == len(rc.passes(c.L)), (name, m)


def test_segment_edges():
    want = {312: (512, 512, 1), 313: (513, 512, 2), 824: (1024, 512, 2), 825: (1025, 512, 3), 999: (1199, 512, 3), 1000: (1200, 512, 3),
            1010: (1212, 512, 3), 27308: (32768, 512, 64), 27309: (32769, 576, 57)}
    for L, (n, sl, ns) in want.items():
        assert rc.cases()[f"segment_{L}"].L == L
        assert (rc.padded_len(L), rc.seg_len(rc.padded_len(L)), rc.n_segments(L)) == (n, sl, ns), L
    assert rc.rand_len(999) == 100 and rc.rand_len(1000) == 100 and rc.rand_len(1010) == 101


@pytest.mark.parametrize("manhattan", MODES)
def test_every_pass_records_a_range_that_survives(table, manhattan):
    seen, second_turn = set(), 0
    for name, c in rc.cases().items():
        ranges, raw, _ = table[name][manhattan]
        mine = rc.passes(c.L)
        idx = _surviving_passes(c.L, ranges, raw)
        seen |= {rc.ALL_PASSES.index(mine[i]) for i in idx}
        second_turn += sum(1 for i in idx if i >= rc.PIPE_WAVES)          # a pass that is some wavefront's second turn in the pipeline
    assert seen == set(range(20)), sorted(set(range(20)) - seen)
    assert second_turn >= 4


@pytest.mark.parametrize("manhattan", MODES)
def test_phase_d_forms(table, manhattan):
    forms = set()
    for name, c in rc.cases().items():
        raw = table[name][manhattan][1]
        cnt = len(raw)
        if c.lists == "lds":
            assert cnt < 6000, (name, cnt)
        else:
            assert cnt > 7000, (name, cnt)
            assert rc.no_cut(raw) == (c.lists == "window"), name
        forms.add(c.lists)
    assert forms == {"lds", "cuts", "window"}
    # the window is refilled at least once, and its last refill is shorter than the window
    assert all(len(table[n][manhattan][1]) > rc.DEDUP_WINDOW + 128 for n, c in rc.cases().items() if c.lists == "window")


@pytest.mark.parametrize("manhattan", MODES)
def test_the_clean_repeats_cross_segment_and_tile_boundaries(table, manhattan):
    for name, start, length in (("clean_6000", 300, 1400), ("clean_30000", 300, 1800)):
        c = rc.cases()[name]
        r, sl = rc.rand_len(c.L), rc.seg_len(rc.padded_len(c.L))
        assert length > 2 * rc.TILE and (start + r) // sl < (start + length + r) // sl
        unit = 7 if name == "clean_6000" else 20
        assert np.array_equal(c.codes[start:start + length - unit], c.codes[start + unit:start + length])
        # ... and a surviving range inside the repeat spans a segment boundary
        ranges = table[name][manhattan][0]
        assert any(start <= s and e <= start + length + 200 and (s + r) // sl < (e + r) // sl for s, e, _, _ in ranges), name
    assert rc.seg_len(rc.padded_len(6000)) == 512 and rc.seg_len(rc.padded_len(30000)) == 576


def test_batches():
    cs, bs = rc.cases(), rc.batches()
    assert all(0 < len(b) <= rc.PARTS_MAX and all(n in cs for n in b) for b in bs.values())
    assert {n for b in bs.values() for n in b} == set(cs)                  # every read runs
    lens = [cs[n].L for n in bs["mixed"]]
    assert 12 in lens and 20482 in lens and 60000 in lens and min(lens) <= 2
    assert bs["mixed_reversed"] == bs["mixed"][::-1] and len(bs["single"]) == 1 and bs["single"][0] in bs["mixed"]
    assert cs[bs["single"][0]].L < max(lens)                                # alone, the read's scratch layout is its own; in the batch, the longest read's
    assert {cs[n].lists for n in bs["mixed"]} == {"lds", "cuts", "window"}


def test_print_the_case_table(table):
    print("\nname L n passes segments | alive ranges cut-free (Manhattan) | alive ranges cut-free (Pearson) | phase D")
    for name, c in rc.cases().items():
        cols = [name, c.L, rc.padded_len(c.L), len(rc.passes(c.L)), rc.n_segments(c.L)]
        for m in MODES:
            ranges, raw, _ = table[name][m]
            cols += ["|", len(raw), len(ranges), rc.no_cut(raw)]
        print(*cols, "|", c.lists)
