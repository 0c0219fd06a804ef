// seed_index.h — the exact seed screen of the catalogue genotype (catalog.hip.inc, mtr_genotype_catalog_device): which q-mers of a read are seeds
// of a flank pattern.  Plain C++, nothing of HIP: the same functions compile into the gfx950 kernels and into a host program
// (tests/seed_index_check.cpp).
//
// The pigeonhole behind it: a pattern p of m >= (K + 1) * q bases has the K + 1 disjoint seeds p[i * q .. i * q + q), i = 0 .. K; a substring of the
// read within K edits of p leaves at least one of them untouched, so that seed occurs in the read exactly.
//   code        a q-mer as 2 bits per base, the first base in the highest of its 2 * q bits (8 <= q <= 16: a uint32_t).
//   text        the device layout: 2 bits per base, first base in the top bits of word 0.  How a word is had is the Load type's business: ld(w) ->
//               word w.  A window loads the word of its first base, and the next one only when it reaches into it: never a word beyond the read's.
//   filter      a bitmap of 2^fbits bits over the TOP bits of the hash: "no" for almost every position of a read without a look at the table.
//   table       open addressing, linear probing over cap = 2^k slots on the LOW bits of the hash; a slot is a distinct code and its run
//               (first, count) in the entries sorted by code; count = 0 marks an empty slot.  The host fills it to at most half.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SI_HD static inline __host__ __device__ __attribute__((always_inline))
#else
#define SI_HD static inline __attribute__((always_inline))
#endif
#define SI_MIN_Q 8
#define SI_MAX_Q 16

struct SiTable {
    const uint32_t *filter; int fbits;      // 2^fbits bits, 32 a word; fbits >= 5
    const uint32_t *key;                    // [cap]
    const int32_t *run;                     // [cap][2]: first, count
    uint32_t cap;                           // a power of two, or 0: no seed at all
};
struct SiRun { int32_t first, count; };

SI_HD int si_seed_offset(int i, int q) { return i * q; }
// the code of codes[0 .. q) (0..3 each)
SI_HD uint32_t si_seed_code(const uint8_t *codes, int q)
{
    uint32_t c = 0;
    for (int t = 0; t < q; t++) c = (c << 2) | (uint32_t)(codes[t] & 3);
    return c;
}
// the code of the text's bases pos .. pos + q; the caller keeps pos + q within the text
template <class Load>
SI_HD uint32_t si_window_code(const Load &ld, int pos, int q)
{
    const int w = pos >> 4, r = pos & 15;
    uint64_t two = (uint64_t)ld(w) << 32;
    if (r + q > 16) two |= (uint64_t)ld(w + 1);
    return (uint32_t)((two << (2 * r)) >> (64 - 2 * q));
}
SI_HD uint32_t si_hash(uint32_t code)
{
    uint32_t h = code * 0x9E3779B1u;
    h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13;
    return h;
}
SI_HD uint32_t si_filter_bit(uint32_t code, int fbits) { return si_hash(code) >> (32 - fbits); }
SI_HD bool si_filter_has(const SiTable &t, uint32_t code)
{
    const uint32_t b = si_filter_bit(code, t.fbits);
    return (t.filter[b >> 5] >> (b & 31)) & 1u;
}
// the run of `code`, count = 0 if it is no seed
SI_HD SiRun si_probe(const SiTable &t, uint32_t code)
{
    SiRun none = { 0, 0 };
    if (t.cap == 0) return none;
    for (uint32_t s = si_hash(code) & (t.cap - 1), n = 0; n < t.cap; s = (s + 1) & (t.cap - 1), n++) {
        const int32_t count = t.run[2 * s + 1];
        if (count == 0) return none;
        if (t.key[s] == code) { const SiRun r = { t.run[2 * s], count }; return r; }
    }
    return none;
}
// the host's side of the table: a distinct code goes in once (count >= 1); false if the table is full
SI_HD bool si_insert(uint32_t *key, int32_t *run, uint32_t cap, uint32_t code, int32_t first, int32_t count)
{
    if (cap == 0) return false;
    for (uint32_t s = si_hash(code) & (cap - 1), n = 0; n < cap; s = (s + 1) & (cap - 1), n++)
        if (run[2 * s + 1] == 0) { key[s] = code; run[2 * s] = first; run[2 * s + 1] = count; return true; }
    return false;
}
SI_HD void si_filter_set(uint32_t *filter, int fbits, uint32_t code)
{
    const uint32_t b = si_filter_bit(code, fbits);
    filter[b >> 5] |= 1u << (b & 31);
}
