// catalog_build.h — what the device build of a prepared locus catalogue (catalog_build.hip.inc, mtr_catalog_create) shares with the host:
// a slot's pattern out of the loci's ASCII, the radix sort's digit and stable rank, the duplicate drop, the table's sizes, a motif's
// reversed 2-bit form.  Plain C++, nothing of HIP: the same functions compile into the gfx950 kernels and into a host program
// (tests/catalog_build_check.cpp).
//   slot        locus * 4 + j: j = 0 the left flank, 1 the right, 2 and 3 their reverse complements (genotype.hip.inc: A, B, rc A, rc B).
//   entry       (code, slot): seed i of the slot's pattern (seed_index.h).  The slots emit theirs in ascending (slot, i) order, so a STABLE
//               sort by code alone leaves every code's entries in ascending slot order, and the copies of one (code, slot) side by side.
//   digit       the sort runs least significant digit first over the 2 * q bits of a code, 8 bits a pass.
//   peers       the lanes of a wavefront that hold the digit of this lane, as a 64-bit mask: the AND over the digit's eight bits of the
//               ballot of that bit or its complement.  A lane's rank among the tile's entries of its digit is what the earlier steps
//               counted plus its peers in lower lanes - no atomic, the same order in every run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CB_HD static inline __host__ __device__ __attribute__((always_inline))
#else
#define CB_HD static inline __attribute__((always_inline))
#endif
#define CB_DIGIT_BITS 8
#define CB_DIGITS 256
#define CB_TILE 1024                    // entries a workgroup of the sort counts and places: 16 steps of a wavefront
#define CB_MAX_M 64                     // the longest flank (FBV_MAX_M)
#define CB_FILTER_MIN_BITS 15           // CAT_FILTER_MIN_BITS, CAT_FILTER_MAX_BITS (catalog.hip.inc)
#define CB_FILTER_MAX_BITS 24

// the code of an ASCII base; -1: none of ACGT
CB_HD int cb_base_code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// the pattern of slot j (0..3) of a locus whose flank `side` = j & 1 is the m letters at `flank`: out[0 .. m) = its codes for j < 2, its
// reverse complement's for j >= 2.  The letters are ACGT (the catalogue's checks come first).
CB_HD void cb_slot_codes(const char *flank, int m, int j, uint8_t *out)
{
    const bool rc = j >= 2;
    for (int t = 0; t < m; t++) {
        const int c = cb_base_code(flank[rc ? m - 1 - t : t]) & 3;
        out[t] = (uint8_t)(rc ? 3 - c : c);
    }
}
// a motif's codes forwards (strand 0) or reverse-complemented (strand 1), as motif_slots lays a slot out
CB_HD void cb_motif_codes(const char *motif, int U, int strand, uint8_t *out)
{
    for (int t = 0; t < U; t++) {
        const int c = cb_base_code(motif[strand ? U - 1 - t : t]) & 3;
        out[t] = (uint8_t)(strand ? 3 - c : c);
    }
}
// mdp_motif_bits (base j at bits 2j) of the reversed codes, from the bits of the codes themselves; U <= 32
CB_HD uint64_t cb_bits_reversed(uint64_t bits, int U)
{
    uint64_t r = 0;
    for (int j = 0; j < U && j < 32; j++) r |= ((bits >> (2 * (U - 1 - j))) & 3) << (2 * j);
    return r;
}

// the sort: passes over a code of q bases, a pass's digit of a key
CB_HD int cb_passes(int q) { return (2 * q + CB_DIGIT_BITS - 1) / CB_DIGIT_BITS; }
CB_HD uint32_t cb_digit(uint32_t key, int pass) { return (key >> (CB_DIGIT_BITS * pass)) & (CB_DIGITS - 1); }
// the peers of a lane whose digit is `digit`: ballot[b] = the lanes whose digit has bit b set, active = the lanes that hold an entry
CB_HD uint64_t cb_peers(const uint64_t *ballot, uint32_t digit, uint64_t active)
{
    uint64_t m = active;
    for (int b = 0; b < CB_DIGIT_BITS; b++) m &= ((digit >> b) & 1) ? ballot[b] : ~ballot[b];
    return m;
}
CB_HD int cb_popc64(uint64_t v) { int n = 0; for (; v; v &= v - 1) n++; return n; }
// a lane's place among its peers, and whether it is the last of them (that lane adds the peers' number to the digit's count)
CB_HD int cb_peer_rank(uint64_t peers, int lane) { return cb_popc64(peers & (((uint64_t)1 << lane) - 1)); }
CB_HD bool cb_peer_last(uint64_t peers, int lane) { return (peers >> lane) == 1; }

// the sorted entries e - 1 and e: e is kept unless it repeats its predecessor; it heads a run where the code changes
CB_HD bool cb_keep(bool first, uint32_t key, int32_t slot, uint32_t prev_key, int32_t prev_slot) { return first || key != prev_key || slot != prev_slot; }
CB_HD bool cb_head(bool first, uint32_t key, uint32_t prev_key) { return first || key != prev_key; }

// the table's slots and the filter's bits for `distinct` codes: catalog_index's rules
CB_HD uint32_t cb_table_cap(uint64_t distinct) { uint32_t cap = 64; while ((uint64_t)cap < 2 * distinct) cap <<= 1; return cap; }
CB_HD int cb_filter_bits(uint64_t distinct)
{
    int fbits = CB_FILTER_MIN_BITS;
    while (fbits < CB_FILTER_MAX_BITS && ((uint64_t)1 << fbits) < 16 * distinct) fbits++;
    return fbits;
}
