"""Loci for the prepared catalogue's tests, from seeded generators: tests/test_catalog_build_ref.py shows from tests/catalog_build_ref.py alone
that they are not degenerate, tests/test_gpu_catalog_prepared.py builds every set on the GPU and compares the device's tables with the reference's.
A set is (loci, K, q): loci = [(A, M, B)] of code arrays, K = max_flank_dist, q = seed_len.

Entries are EMITTED four to a locus and seed (a flank, the other flank, their reverse complements): the emitted totals either side of a
wavefront, of 256 and of a sort tile are 60 / 64 / 68, 252 / 256 / 260 and 1020 / 1024 / 1028 (the last puts one locus' entries into a second
tile).  The KEPT entries may be of any number: seeds sit at i * q from a pattern's start, so in a flank of more than (K + 1) * q bases the
reverse complement's seeds cover the flank's other end, and a flank X + X + three bases (K = 1, q = 8) drops one duplicate in its own slot
and none in its reverse complement's.  The sets kept_63 .. kept_1025 have exactly that many kept entries - the sizes of `ent` and of the
compaction's scans - and distinct_63 .. distinct_257 that many DISTINCT CODES, a lane each of the table's kernel, through flanks that are
their own reverse complement."""
import numpy as np

from tests import catalog_build_ref as cbr
from tests import catalog_cases as cc

MANY = 300                                       # catalog_cases.MANY extended: loci that share both flanks, a code of more than 256 slots
MOTIF_LENGTHS = (1, 4, 5, 16, 17, 32, 33, 499)
EMITTED = (60, 64, 68, 252, 256, 260, 1020, 1024, 1028)
DISTINCT = (63, 64, 65, 255, 256, 257)
KEPT = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)       # kept entries: K = 1, q = 8, eight emitted a locus, one dropped per flank X + X + 3 bases
SORT_TILE = 1024                                 # CB_TILE of mtr_amd/csrc/catalog_build.h


def _code(p):
    c = 0
    for v in p:
        c = c * 4 + int(v)
    return c


def _rc(p):
    return (3 - np.asarray(p, np.uint8))[::-1]


def _uncode(c, q):
    return np.array([(c >> (2 * (q - 1 - t))) & 3 for t in range(q)], np.uint8)


def filter_pair(q: int = 8):
    """two distinct q-mer codes, neither the other's reverse complement nor its own, whose hashes share their top 15 bits: one filter bit"""
    seen = {}
    for c in range(1, 1 << (2 * q)):
        p = _uncode(c, q)
        if _code(_rc(p)) == c:
            continue
        b = int(cbr.si_hash(np.array([c]))[0]) >> (32 - cbr.FILTER_MIN_BITS)
        if b in seen and _code(_rc(_uncode(seen[b], q))) != c:
            return seen[b], c
        seen.setdefault(b, c)
    raise AssertionError("no pair found")


def _distinct_flanks(rng, n_flanks, n_pal, q=8):
    """n_flanks flanks of q bases whose codes and reverse complements' codes are all different, but that the first n_pal are their own reverse
    complement: 2 * n_flanks - n_pal distinct codes"""
    used, out = set(), []
    while len(out) < n_flanks:
        if len(out) < n_pal:
            half = rng.randint(0, 4, size=q // 2).astype(np.uint8)
            p = np.concatenate([half, _rc(half)])
        else:
            p = rng.randint(0, 4, size=q).astype(np.uint8)
        c, r = _code(p), _code(_rc(p))
        if c in used or r in used or ((c == r) != (len(out) < n_pal)):
            continue
        used |= {c, r}
        out.append(p)
    return out


def sets():
    """-> {name: (loci, K, q)}"""
    out = {}
    for K, q in cc.KQ:
        out[f"cases_K{K}_q{q}"] = (cc.cases(K, q)[0], K, q)
    rng = np.random.RandomState(4242)
    seq = lambda n: rng.randint(0, 4, size=n).astype(np.uint8)      # noqa: E731
    A, B = seq(64), seq(64)
    out["many"] = ([(A, seq(2 + j % 7), B) for j in range(MANY)], 3, 16)
    # q = 16, K = 1: a flank of 32 A (its two seeds are equal: code 0, and all ones in the reverse complement), a flank of one seed twice, every
    # motif length at a border, flanks of 32 (the narrow word), 33 and 64 bases (the wide one)
    twice = seq(16)
    edge = [(np.zeros(32, np.uint8), seq(MOTIF_LENGTHS[0]), np.concatenate([twice, twice]))]
    edge += [(seq((32, 33, 64)[k % 3]), seq(U), seq((64, 32, 33)[k % 3])) for k, U in enumerate(MOTIF_LENGTHS[1:])]
    out["edge_q16"] = (edge, 1, 16)
    out["one_locus"] = ([(np.tile(seq(8), 3), seq(3), seq(40))], 2, 8)               # the left flank is one seed three times
    c1, c2 = filter_pair(8)
    out["one_filter_bit"] = ([(_uncode(c1, 8), seq(3), seq(8)), (_uncode(c2, 8), seq(4), seq(8))] + [(seq(8), seq(2), seq(9)) for _ in range(10)], 0, 8)
    out["narrow_only"] = ([(seq(12 + k % 21), seq(1 + k % 9), seq(32 - k % 21)) for k in range(9)], 0, 12)
    out["wide_only"] = ([(seq(33 + k % 32), seq(1 + k % 9), seq(64 - k % 32)) for k in range(9)], 1, 16)
    for total in EMITTED:
        n = total // 4
        out[f"emitted_{total}"] = ([(seq(12 + (5 * k) % 40), seq(1 + k % 6), seq(12 + (7 * k) % 53)) for k in range(n)], 0, 12)
    for total in DISTINCT:
        n_pal = (-total) % 4 if total % 4 else 0
        n_flanks = (total + n_pal) // 2
        fl = _distinct_flanks(rng, n_flanks, n_pal)
        order = rng.permutation(n_flanks)
        out[f"distinct_{total}"] = ([(fl[order[2 * k]], seq(1 + k % 5), fl[order[2 * k + 1]]) for k in range(n_flanks // 2)], 0, 8)
    for total in KEPT:
        n = (total + 7) // 8
        drop = 8 * n - total                                         # 0 .. 7 flanks of a seed twice and three more bases
        flanks = []
        for k in range(2 * n):
            X = seq(8)
            flanks.append(np.concatenate([X, X, seq(3)]) if k < drop else seq(16 + k % 9))
        order = rng.permutation(2 * n)
        out[f"kept_{total}"] = ([(flanks[order[2 * k]], seq(1 + k % 5), flanks[order[2 * k + 1]]) for k in range(n)], 1, 8)
    FA, FB = rng.randint(0, 4, size=(17000, 16)).astype(np.uint8), rng.randint(0, 4, size=(17000, 16)).astype(np.uint8)
    out["slots_beyond_2_16"] = ([(FA[l], seq(1 + l % 4), FB[l]) for l in range(17000)], 0, 16)
    return out
