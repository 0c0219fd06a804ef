// unit_motif.h — the canonical motif of one repeat unit: the unit grouped over rotation and strand.  Plain C++, nothing of HIP: the same
// function compiles into the gfx950 kernels (report_motif.hip.inc) and into a host program (tests/unit_motif_check.cpp).
//
// For a unit u of p bytes over ACGT (include/mtr_hip.h, "the motif catalogue"):
//   rc(u)       the reverse complement;  rot(s, r)[i] = s[(i + r) mod p];  strings compare bytewise (A < C < G < T)
//   canon(u)    the smallest of the 2p strings rot(u, r), rot(rc(u), r);  strand = 0 if a rot(u, r) attains it (the forward strand wins a
//               tie), else 1;  rotation = the smallest r on that strand that attains it
//   motif_len   the smallest divisor d of p with rot(canon, d) == canon;  the motif is canon[0 .. d)
//   p == 0      strand = rotation = motif_len = 0 and the empty motif
// The least rotation of a strand is the constant-memory two-pointer walk ("minimal representation"): candidates i < j, k bases of both
// known equal; a mismatch throws out the larger candidate and the k starts behind it, which cannot win either.  O(p) steps, no failure
// array, no recursion, no memory of its own.  It ends on the SMALLEST start of a least rotation: of two equal rotations the walk keeps
// the smaller start (k reaches p).  One walk per strand (um_least_rotation: the two are independent, and the kernel gives them to two
// lanes), then one comparison of the two winners and the rest (unit_motif_from).  unit_motif() is the three in a row.
// The primitive period is read off the unit itself - rotation and reverse complement keep it - by testing the divisors of p.
#pragma once
#include "mtr_common.h"

#define UM_HD static inline __host__ __device__ __attribute__((always_inline))

struct UnitMotif { int strand, rotation, motif_len; };

UM_HD int um_comp(int c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }
// base i of the strand: u itself, or its reverse complement
// (one load and selects whatever the strand: lanes on different strands do not diverge)
UM_HD int um_base(const uint8_t *u, int p, int strand, int i) { const int c = u[strand ? p - 1 - i : i]; return strand ? um_comp(c) : c; }

// the smallest r with rot(s, r) least among the rotations of s = strand `strand` of u;  p >= 1
UM_HD int um_least_rotation(const uint8_t *u, int p, int strand)
{
    int i = 0, j = 1, k = 0;
    while (j < p && k < p) {                               // i < j always
        int a = i + k, b = j + k;
        a -= a >= p ? p : 0; b -= b >= p ? p : 0;
        const int ca = um_base(u, p, strand, a), cb = um_base(u, p, strand, b);
        if (ca == cb) { k++; continue; }
        if (ca > cb) { i += k + 1; if (i <= j) i = j++; else { const int t = i; i = j; j = t; } }     // starts i .. i + k all lose; keep i < j
        else j += k + 1;
        k = 0;
    }
    return i;
}

// FNV-1a over motif_len (four bytes, low first) and the motif's bytes
#define UM_HASH_SEED 0xcbf29ce484222325ull
#define UM_HASH_PRIME 0x100000001b3ull
UM_HD uint64_t um_hash_byte(uint64_t h, int c) { return (h ^ (uint64_t)(c & 0xff)) * UM_HASH_PRIME; }
UM_HD uint64_t um_hash_len(int d)
{
    uint64_t h = UM_HASH_SEED;
    for (int q = 0; q < 4; q++) h = um_hash_byte(h, d >> (8 * q));
    return h;
}
// where the grouping starts to probe for a motif in a table of mask + 1 slots (a power of two)
UM_HD uint32_t um_start_slot(uint64_t h, uint32_t mask) { return (uint32_t)(h ^ (h >> 32)) & mask; }

// The motif of u[0 .. p), 0 <= p <= 500, given the least rotations rf of u and rr of rc(u) (um_least_rotation; not looked at for p == 0).
// motif (may be NULL) receives motif_len bytes, hash (may be NULL) the hash of (motif_len, motif).
UM_HD UnitMotif unit_motif_from(const uint8_t *u, int p, int rf, int rr, uint8_t *motif, uint64_t *hash)
{
    UnitMotif m = { 0, 0, 0 };
    if (p <= 0) { if (hash) *hash = um_hash_len(0); return m; }
    int cmp = 0;                                            // rot(u, rf) against rot(rc(u), rr)
    for (int t = 0, a = rf, b = rr; t < p && cmp == 0; t++) {
        cmp = um_base(u, p, 0, a) - um_base(u, p, 1, b);
        a = a + 1 == p ? 0 : a + 1; b = b + 1 == p ? 0 : b + 1;
    }
    m.strand = cmp <= 0 ? 0 : 1;
    m.rotation = m.strand ? rr : rf;
    int d = p;                                              // the smallest divisor of p that is a period of u
    for (int c = 1; c <= p / 2; c++) {
        if (p % c) continue;
        bool per = true;
        for (int t = 0; t + c < p && per; t++) per = u[t] == u[t + c];
        if (per) { d = c; break; }
    }
    m.motif_len = d;
    uint64_t h = um_hash_len(d);
    for (int t = 0, a = m.rotation; t < d; t++) {
        const int c = um_base(u, p, m.strand, a);
        if (motif) motif[t] = (uint8_t)c;
        h = um_hash_byte(h, c);
        a = a + 1 == p ? 0 : a + 1;
    }
    if (hash) *hash = h;
    return m;
}

// The motif of u[0 .. p), 0 <= p <= 500: the single definition.
UM_HD UnitMotif unit_motif(const uint8_t *u, int p, uint8_t *motif, uint64_t *hash)
{
    const int rf = p > 0 ? um_least_rotation(u, p, 0) : 0, rr = p > 0 ? um_least_rotation(u, p, 1) : 0;
    return unit_motif_from(u, p, rf, rr, motif, hash);
}
