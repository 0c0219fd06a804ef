"""The prepared catalogue's case sets (tests/catalog_build_cases.py) are not degenerate: from the reference alone (tests/catalog_build_ref.py),
each thing the device build can get wrong occurs in them, by count.  CPU only."""
import numpy as np
import pytest

from tests import catalog_build_cases as cbc
from tests import catalog_build_ref as cbr


@pytest.fixture(scope="module")
def built():
    return {name: (cbr.build(loci, K, q), loci, K, q) for name, (loci, K, q) in cbc.sets().items()}


def test_a_duplicate_entry_must_be_dropped(built):
    for name in ("edge_q16",):
        ref = built[name][0]
        assert ref.n_entries_emitted - len(ref.ent) >= 4, name          # two flanks of two equal seeds, and their reverse complements
    assert sum(ref.n_entries_emitted > len(ref.ent) for ref, *_ in built.values()) >= 2


def test_codes_shared_by_more_than_64_and_more_than_256_slots(built):
    assert 64 < built["cases_K1_q8"][0].count.max() <= 256
    assert built["many"][0].count.max() == cbc.MANY > 256


def test_two_codes_share_a_table_slot_and_two_share_a_filter_bit(built):
    ref = built["one_filter_bit"][0]
    bits = cbr.si_hash(ref.codes) >> np.uint64(32 - ref.fbits)
    assert len(np.unique(bits)) < len(ref.codes) and ref.fbits == cbr.FILTER_MIN_BITS
    assert int(sum(bin(int(w)).count("1") for w in ref.filter)) == len(np.unique(bits))
    homes = 0
    for ref, *_ in built.values():
        home = cbr.si_hash(ref.codes) & np.uint64(ref.cap - 1)
        homes += len(ref.codes) - len(np.unique(home))
    assert homes >= 100
    for name in ("cases_K3_q16", "distinct_257", "slots_beyond_2_16"):
        ref = built[name][0]
        assert len(np.unique(cbr.si_hash(ref.codes) & np.uint64(ref.cap - 1))) < len(ref.codes), name


def test_code_zero_and_the_code_of_all_ones_rule_out_a_sentinel(built):
    ref, _, K, q = built["edge_q16"]
    assert q == 16 and ref.codes[0] == 0 and ref.codes[-1] == 0xFFFFFFFF


def test_both_ends_of_the_seed_lengths_and_one_locus(built):
    qs = {q for _, _, _, q in built.values()}
    assert {8, 16} <= qs and 12 in qs
    assert len(built["one_locus"][1]) == 1


def test_totals_either_side_of_a_wavefront_256_and_a_sort_tile(built):
    for total in cbc.EMITTED:
        assert built[f"emitted_{total}"][0].n_entries_emitted == total
    assert cbc.SORT_TILE - 4 in cbc.EMITTED and cbc.SORT_TILE in cbc.EMITTED and cbc.SORT_TILE + 4 in cbc.EMITTED
    for total in cbc.KEPT:                                           # the kept entries, odd totals among them: `ent` and the compaction's scans
        ref = built[f"kept_{total}"][0]
        assert len(ref.ent) == total and ref.n_entries_emitted == 8 * ((total + 7) // 8)
    assert {63, 64, 65, 255, 256, 257, cbc.SORT_TILE + 1} <= set(cbc.KEPT)
    for total in cbc.DISTINCT:
        assert len(built[f"distinct_{total}"][0].codes) == total
    # the table's size changes between them: 2 * distinct crosses a power of two
    assert built["distinct_64"][0].cap == 128 and built["distinct_65"][0].cap == 256 and built["distinct_256"][0].cap == 512 and built["distinct_257"][0].cap == 1024


def test_slot_numbers_beyond_16_bits_and_more_than_one_filter_size(built):
    ref = built["slots_beyond_2_16"][0]
    assert int(ref.ent.max()) > 1 << 16 and ref.n_entries_emitted > 60 * cbc.SORT_TILE
    assert ref.fbits > cbr.FILTER_MIN_BITS


def test_both_flank_words(built):
    short = lambda name: built[name][0].plen <= 32      # noqa: E731
    assert short("narrow_only").all() and not short("wide_only").any()
    assert short("edge_q16").any() and not short("edge_q16").all()
    assert {32, 33, 64} <= set(built["edge_q16"][0].plen.tolist())


def test_every_motif_length_at_a_border(built):
    ref = built["edge_q16"][0]
    assert tuple(ref.ulen.tolist()) == cbc.MOTIF_LENGTHS
    long = ref.ulen > 32
    assert (ref.variant_bits.reshape(-1, 4)[long] == 0).all() and (ref.variant_bits.reshape(-1, 4)[~long][:, 0] == ref.unit_bits[0::2][~long]).all()


def test_the_reference_is_consistent(built):
    """the runs tile the entries, every code's slots ascend, and probing a table built in any order finds every run"""
    for name, (ref, loci, K, q) in built.items():
        assert ref.first[0] == 0 and (ref.first[1:] == ref.first[:-1] + ref.count[:-1]).all() and ref.first[-1] + ref.count[-1] == len(ref.ent), name
        assert (ref.pairs[1:] > ref.pairs[:-1]).all(), name
        assert ref.cap >= 2 * len(ref.codes) and ref.cap & (ref.cap - 1) == 0
    ref = built["distinct_257"][0]
    key, run = np.zeros(ref.cap, np.uint32), np.zeros((ref.cap, 2), np.int32)
    for c, f, n in zip(ref.codes[::-1].tolist(), ref.first[::-1].tolist(), ref.count[::-1].tolist()):      # (an order that is not the host's)
        s = int(cbr.si_hash(np.array([c]))[0]) & (ref.cap - 1)
        while run[s, 1]:
            s = (s + 1) & (ref.cap - 1)
        key[s], run[s] = c, (f, n)
    first, count = cbr.probe(key, run, ref.cap, ref.codes)
    assert (first == ref.first).all() and (count == ref.count).all()
    absent = np.setdiff1d(np.arange(1 << 16, dtype=np.uint32), ref.codes)[:500]
    assert (cbr.probe(key, run, ref.cap, absent)[1] == 0).all()
