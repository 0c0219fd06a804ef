"""A prepared catalogue by definition, in numpy: what mtr_catalog_create must hold for loci = [(A, M, B)] of code arrays (0..3), max_flank_dist K
and seed_len q.  Nothing here sorts by digits or probes a table to build one: the entries are the sorted distinct (code, slot) pairs, the runs
their groups by code, the filter the set of the codes' bits, the table's sizes their rule; tests/test_gpu_catalog_prepared.py compares the
device's tables with these, and probes the device's table with probe() below (seed_index.h's si_probe).
  slot     4 * locus + j: j = 0 the left flank A, 1 the right flank B, 2 and 3 their reverse complements
  seed i   the q bases from i * q of a slot's pattern, i = 0 .. K, as a code: first base in the highest of the 2 * q bits"""
from typing import NamedTuple

import numpy as np

FILTER_MIN_BITS, FILTER_MAX_BITS = 15, 24
M32 = np.uint64(0xFFFFFFFF)


def si_hash(code):
    """seed_index.h's si_hash, on uint32 values held in uint64 arrays"""
    h = (np.asarray(code, np.uint64) * np.uint64(0x9E3779B1)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x85EBCA77)) & M32
    h ^= h >> np.uint64(13)
    return h


def table_cap(distinct: int) -> int:
    cap = 64
    while cap < 2 * distinct:
        cap <<= 1
    return cap


def filter_bits(distinct: int) -> int:
    fbits = FILTER_MIN_BITS
    while fbits < FILTER_MAX_BITS and (1 << fbits) < 16 * distinct:
        fbits += 1
    return fbits


def _by_length(seqs):
    """-> [(m, indices, rows [len(indices), m])]: the sequences grouped by their length"""
    lens = np.array([len(s) for s in seqs])
    out = []
    for m in np.unique(lens):
        idx = np.nonzero(lens == m)[0]
        out.append((int(m), idx, np.stack([np.asarray(seqs[i], np.uint8) for i in idx]) if m else np.zeros((len(idx), 0), np.uint8)))
    return out


def slot_patterns(loci):
    """the 4 * n patterns in slot order"""
    pats = []
    for A, _, B in loci:
        A, B = np.asarray(A, np.uint8), np.asarray(B, np.uint8)
        pats += [A, B, (3 - A)[::-1], (3 - B)[::-1]]
    return pats


class Catalog(NamedTuple):
    ent: np.ndarray        # int32 [E]: the slots of the sorted distinct (code, slot)
    codes: np.ndarray      # uint32 [distinct] ascending
    first: np.ndarray      # int32 [distinct]: a code's run in ent
    count: np.ndarray      # int32 [distinct]
    cap: int
    fbits: int
    filter: np.ndarray     # uint32 [2^fbits / 32]
    plen: np.ndarray       # int32 [4n]
    masks: np.ndarray      # uint64 [4n, 8]: A, C, G, T of the pattern, then of the reversed pattern
    units: np.ndarray      # uint8: per locus M then rc M
    unit_off: np.ndarray   # int32 [2n + 1]
    unit_bits: np.ndarray  # uint64 [2n]: base j of the slot at bits 2j, the first 32 bases
    variant_bits: np.ndarray   # uint64 [4n]: M, reversed M, rc M, reversed rc M; 0 for a motif over 32 bases
    ulen: np.ndarray       # int32 [n]
    n_entries_emitted: int  # 4n * (K + 1), duplicates included
    pairs: np.ndarray      # uint64 [E]: code << 32 | slot, ascending


def _bits(rows):
    """[r, U] codes -> uint64 [r]: base j at bits 2j, the first 32 bases"""
    out = np.zeros(rows.shape[0], np.uint64)
    for j in range(min(rows.shape[1], 32)):
        out |= rows[:, j].astype(np.uint64) << np.uint64(2 * j)
    return out


def build(loci, K: int, q: int) -> Catalog:
    n = len(loci)
    pats = slot_patterns(loci)
    S = 4 * n
    plen = np.array([len(p) for p in pats], np.int32)
    assert plen.min() >= (K + 1) * q and plen.max() <= 64 and 8 <= q <= 16 and K >= 0
    masks = np.zeros((S, 8), np.uint64)
    pairs = []
    for m, idx, P in _by_length(pats):
        for i in range(K + 1):
            code = np.zeros(len(idx), np.uint64)
            for t in range(q):
                code = (code << np.uint64(2)) | P[:, i * q + t].astype(np.uint64)
            pairs.append((code << np.uint64(32)) | idx.astype(np.uint64))
        for rev in (0, 1):
            Q = P[:, ::-1] if rev else P
            for c in range(4):
                v = np.zeros(len(idx), np.uint64)
                for i in range(m):
                    v |= (Q[:, i] == c).astype(np.uint64) << np.uint64(i)
                masks[idx, 4 * rev + c] = v
    emitted = np.concatenate(pairs)
    uniq = np.unique(emitted)                                   # sorted by (code, slot), distinct
    code_of = (uniq >> np.uint64(32)).astype(np.uint32)
    ent = (uniq & M32).astype(np.int32)
    codes, first, count = np.unique(code_of, return_index=True, return_counts=True)
    distinct = len(codes)
    cap, fbits = table_cap(distinct), filter_bits(distinct)
    bit = si_hash(codes) >> np.uint64(32 - fbits)
    filt = np.zeros((1 << fbits) // 32, np.uint32)
    np.bitwise_or.at(filt, (bit >> np.uint64(5)).astype(np.int64), (np.uint64(1) << (bit & np.uint64(31))).astype(np.uint32))
    # the motif tables
    motifs = [np.asarray(M, np.uint8) for _, M, _ in loci]
    ulen = np.array([len(M) for M in motifs], np.int32)
    unit_off = np.zeros(2 * n + 1, np.int64)
    unit_off[1::2] = ulen
    unit_off[2::2] = ulen
    unit_off = np.cumsum(unit_off).astype(np.int32)
    units = np.zeros(int(unit_off[-1]), np.uint8)
    unit_bits, variant_bits = np.zeros(2 * n, np.uint64), np.zeros(4 * n, np.uint64)
    for U, idx, P in _by_length(motifs):
        RC = (3 - P)[:, ::-1]
        cols = np.arange(U)
        units[unit_off[2 * idx][:, None] + cols] = P
        units[unit_off[2 * idx + 1][:, None] + cols] = RC
        unit_bits[2 * idx], unit_bits[2 * idx + 1] = _bits(P), _bits(RC)
        if U <= 32:
            for k, V in enumerate((P, P[:, ::-1], RC, RC[:, ::-1])):
                variant_bits[4 * idx + k] = _bits(V)
    return Catalog(ent, codes.astype(np.uint32), first.astype(np.int32), count.astype(np.int32), cap, fbits, filt, plen, masks, units, unit_off, unit_bits, variant_bits, ulen,
                   S * (K + 1), uniq)


def probe(key, run, cap: int, codes):
    """seed_index.h's si_probe of every code on a dumped table: -> (first, count) arrays, count = 0 where the code is no seed.  Bounded by cap."""
    codes = np.asarray(codes, np.uint64)
    s = (si_hash(codes) & np.uint64(cap - 1)).astype(np.int64)
    first, count = np.zeros(len(codes), np.int64), np.zeros(len(codes), np.int64)
    todo = np.arange(len(codes))
    run = np.asarray(run).reshape(cap, 2)
    for _ in range(cap):
        if len(todo) == 0:
            break
        at = s[todo]
        c = run[at, 1]
        hit = (c != 0) & (np.asarray(key)[at].astype(np.uint64) == codes[todo])
        first[todo[hit]], count[todo[hit]] = run[at[hit], 0], c[hit]
        go = (c != 0) & ~hit
        todo = todo[go]
        s[todo] = (s[todo] + 1) & (cap - 1)
    return first, count
