"""The CPU oracle's unit search, pinned so that it can answer for any (read, window, k) where the reference does not exist
(the stage tests of the kernels' unit search, trace events 2 and 8, are to ask it):
  (a) its level-2 capture of 3_5 and synth_2k is the reference's own recorded G2 stream (tests/golden/*.default.l2.jsonl.gz), units included;
  (b) mtro_search_unit, the stand-alone export, reproduces every G2 line of a level-3 capture of the seeded set of tests/unit_search_set.py;
  (c) mtro_walk, the stand-alone walk, gives the unit of every search that kept one: the first closing walk of one of the two directions;
  and the set reaches every k-mer table layout of the kernels with the numbers of events the stage tests rely on."""
import gzip
import json
import os

import pytest

from tests import golden_util as gu
from tests import unit_search_set as uss
from tests.oracle_binding import Oracle


@pytest.mark.parametrize("name,lines", [("3_5", 68), ("synth_2k", 667)])
def test_level2_capture_is_the_references_G2_stream(name, lines):
    reads = [c for _, c in gu.read_fasta(gu.input_path(name))]
    got = [json.dumps(g, separators=(",", ":")) for g in uss.capture_g2(reads, level=2)]
    with gzip.open(os.path.join(gu.GOLDEN, f"{name}.default.l2.jsonl.gz"), "rt") as fh:
        want = fh.read().splitlines()
    assert len(want) == lines
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, f"{name}: G2 line {i} differs:\n got  {x[:300]}\n want {y[:300]}"
    assert len(got) == len(want)


@pytest.fixture(scope="module")
def oracle():
    o = Oracle()
    yield o
    o.close()


def _sets():
    return [("small", uss.small_reads(), uss.oracle_g2_small()), ("wide", uss.wide_reads(), uss.oracle_g2_wide())]


def test_search_unit_export_replays_the_level3_capture(oracle):
    n = 0
    for name, reads, events in _sets():
        for g in events:
            r = oracle.search_unit(reads[g["rd"]], g["qs"], g["qe"], g["k"])
            got = {f: r[f] for f in ("found", *uss.FIELDS, "unit")}
            want = {f: g[f] for f in ("found", *uss.FIELDS, "unit")}
            assert got == want, (name, g["rd"], g["qs"], g["qe"], g["k"])
            assert (r["max_freq"] > 5) or (not g["found"] and g["period"] == -1)      # consensus.c:532: no walk unless a node occurs more than 5 times
            n += 1
    assert n > 30000


def test_walk_export_gives_the_unit_of_every_search_that_kept_one(oracle):
    """search_De_Bruijn_graph tries the seeds in order, forward then backward, and aligns the first walk of each direction that closes
    (consensus.c:536-579): the unit a search kept is that of one of these two walks."""
    n = 0
    for name, reads, events in _sets():
        for g in events:
            if g["period"] <= 0:
                continue
            codes = reads[g["rd"]]
            seeds = oracle.search_unit(codes, g["qs"], g["qe"], g["k"])["seeds"]
            first = []
            for backward in (False, True):
                for seed in seeds:
                    period, unit = oracle.walk(codes, g["qs"], g["qe"], g["k"], backward, seed)
                    if period:
                        first.append((period, unit))
                        break
            assert (g["period"], g["unit"]) in first, (name, g["rd"], g["qs"], g["qe"], g["k"], g["period"], first)
            n += 1
    assert n > 1000                 # (of the ~2 150 searches whose last walk closed, about half keep a unit: the others' alignments fail the selection)


def test_the_set_reaches_every_table_layout():
    """The floors stage tests of the unit search stand on, from the oracle's events alone, and the counts DESIGN.md quotes."""
    events = uss.oracle_g2_small() + uss.oracle_g2_wide()
    cnt = uss.assert_every_regime_is_reached(events)
    assert {name: (c["found"], c["not_found"]) for name, c in cnt.items()} == uss.DOCUMENTED_COUNTS


def test_layout_rule():
    assert [uss.layout(w, k) for w, k in ((65535, 6), (65536, 6), (65536, 5), (1400, 7), (1400, 10), (1400, 11), (1401, 7), (1401, 11), (1401, 6))] == \
        ["direct", "split_global", "split_global", "packed", "packed", "split_lds", "split_global", "split_global", "direct"]
