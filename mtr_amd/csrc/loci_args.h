// loci_args.h — what the text and the lengths of a set of loci decide, once for every call that takes loci (the genotype, the partial genotype,
// their catalogue forms, mtr_catalog_create) and, sequence by sequence, for the motif and the flank searches: the checks with their refusals'
// words, the arrays that lengths alone fix, the codes of flanks and motifs.  Plain C++17, nothing of HIP: the host side of the library and a
// host-only program (tests/loci_args_check.cpp) compile the same functions.
//   loci        seqs[seq_off[k] .. seq_off[k + 1]), k = 3 * locus + which: the left flank, the motif, the right flank.
//   key         the place of a refusal, ordered as the checks go: all motifs by locus, then the flanks locus by locus, left before right; within
//               one sequence its length before its bytes.  bit 62: a flank; bits 10..61: the motif's locus, or 2 * locus + side; bits 0..9: the
//               byte's position + 1, 0 for the length.  The smallest key of a set of loci is the refusal a sequential walk meets first, whoever
//               found it: la_lengths finds the lengths', la_first_bad_letter - or the device (catb_bad_key, mtr_k_catb_check) - the bytes'.
//   refusal     every function here that checks returns true, or false with the reason in `err`; the status is the caller's (MTR_ERR_BAD_ARG).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mtr_common.h"
#include "catalog_build.h"
#include "flank_bv.h"
#include "motif_dp.h"
#include "seed_index.h"

#define LA_NO_KEY (~0ull)
static_assert(FBV_MAX_M == CB_MAX_M, "one longest flank");

inline unsigned long long la_key(int is_flank, int64_t index, int64_t t) { return ((unsigned long long)is_flank << 62) | ((unsigned long long)index << 10) | (unsigned long long)(t + 1); }
inline bool la_key_is_flank(unsigned long long key) { return (key >> 62) & 1; }
inline int64_t la_key_index(unsigned long long key) { return (int64_t)((key >> 10) & (((unsigned long long)1 << 52) - 1)); }
inline int64_t la_key_t(unsigned long long key) { return (int64_t)(key & 1023) - 1; }                        // -1: the length
// the sequence of the loci (k of seq_off) a key speaks of, and its name in a refusal
inline size_t la_key_seq(unsigned long long key) { const size_t i = (size_t)la_key_index(key); return la_key_is_flank(key) ? 3 * (i / 2) + 2 * (i % 2) : 3 * i + 1; }
inline std::string la_flank_name(int64_t l, int side) { return "locus " + std::to_string(l) + ", " + (side ? "right" : "left") + " flank"; }
inline std::string la_motif_name(int64_t m) { return "motif " + std::to_string(m); }
inline std::string la_key_name(unsigned long long key) { const int64_t i = la_key_index(key); return la_key_is_flank(key) ? la_flank_name(i / 2, (int)(i % 2)) : la_motif_name(i); }

// one sequence: whether its length is a flank's (1 .. FBV_MAX_M) or a motif's (1 .. MTRC_MAX_PERIOD - 1), its first byte that is none of ACGT
// (len: none), and the two together as the t of a key: -1 the length, len nothing to refuse
inline bool la_length_ok(bool is_flank, int64_t len) { return len >= 1 && (is_flank ? len <= FBV_MAX_M : len < MTRC_MAX_PERIOD); }
inline int64_t la_first_bad_byte(const char *s, int64_t len) { int64_t t = 0; while (t < len && cb_base_code(s[t]) >= 0) t++; return t; }
inline int64_t la_seq_check(bool is_flank, const char *s, int64_t len) { return la_length_ok(is_flank, len) ? la_first_bad_byte(s, len) : -1; }
// the words of the refusal at t (-1 .. len - 1) of the sequence `what`
inline std::string la_refusal(const std::string &what, bool is_flank, int64_t t, const char *s, int64_t len)
{
    if (t < 0) return what + ": length " + std::to_string(len) + " outside 1.." + std::to_string(is_flank ? FBV_MAX_M : MTRC_MAX_PERIOD - 1);
    return what + ": byte " + std::to_string((int)(unsigned char)s[t]) + " at " + std::to_string(t) + " is none of ACGT";
}
// the same from a key of the loci; false: the key names no byte of its sequence (err is left alone)
inline bool la_key_refusal(unsigned long long key, const char *seqs, const int64_t *seq_off, std::string &err)
{
    const size_t k = la_key_seq(key);
    const int64_t len = seq_off[k + 1] - seq_off[k], t = la_key_t(key);
    if (t >= len) return false;
    err = la_refusal(la_key_name(key), la_key_is_flank(key), t, seqs + seq_off[k], len);
    return true;
}

// ---- the checks ----
inline bool la_refuse(std::string &err, const std::string &why) { err = why; return false; }
inline bool la_check_offsets(const char *seqs, const int64_t *seq_off, int32_t n_loci, std::string &err)
{
    if (n_loci <= 0) return la_refuse(err, "n_loci = " + std::to_string(n_loci) + ": at least one locus is needed");
    if (!seqs || !seq_off) return la_refuse(err, "seqs or seq_off is NULL");
    if (n_loci > INT32_MAX / 4) return la_refuse(err, "more than 2^29 - 1 loci");
    for (int32_t k = 0; k < 3 * n_loci; k++)
        if (seq_off[k + 1] < seq_off[k]) return la_refuse(err, "seq_off decreases at locus " + std::to_string(k / 3) + " (sequence " + std::to_string(k % 3) + ")");
    return true;
}
inline bool la_check_scores(int32_t gain, int32_t mismatch, int32_t indel, std::string &err)
{
    if (gain < 1 || gain > 5) return la_refuse(err, "gain = " + std::to_string(gain) + " outside 1..5");
    if (mismatch < 1 || mismatch > 3) return la_refuse(err, "mismatch = " + std::to_string(mismatch) + " outside 1..3");
    return (indel >= 1 && indel <= 3) || la_refuse(err, "indel = " + std::to_string(indel) + " outside 1..3");
}
// (the slots and their codes are indexed with 32 bits on the two strands)
inline bool la_check_motif_total(int64_t n_motifs, int64_t motif_bases, std::string &err) { return (n_motifs <= INT32_MAX / 2 && motif_bases <= INT32_MAX / 2) || la_refuse(err, "more than 2^30 - 1 motifs or motif bases"); }

// What the lengths of checked offsets decide (la_check_offsets comes first).  A refused length is never built: its offsets only stay 32-bit.
struct LociLengths {
    std::vector<int64_t> mot_off;                       // [n_loci + 1]: the motifs side by side, as the motif search takes them
    std::vector<int32_t> unit_off;                      // [2 * n_loci + 1]: the single-strand motif slots, 2 * l as given, 2 * l + 1 reverse-complemented
    std::vector<int32_t> plen, ulen;                    // [4 * n_loci]: the flank slots' lengths (A, B, rc A, rc B); [n_loci]: the motifs'
    std::vector<int64_t> off;                           // [3 * n_loci + 1]: seq_off from 0
    int64_t n_short = 0, n_long = 0;                    // flank slots of at most / of more than 32 bases
    int64_t first_long_motif = -1;                      // the first locus whose motif has more than MDP_MAX_U bases
    unsigned long long first_bad_length = LA_NO_KEY;    // the smallest key of a refused length
};
inline void la_lengths(const int64_t *seq_off, int32_t n_loci, LociLengths &o)
{
    const size_t nl = (size_t)n_loci;
    o = LociLengths();
    o.mot_off.assign(nl + 1, 0); o.unit_off.assign(2 * nl + 1, 0); o.plen.resize(4 * nl); o.ulen.resize(nl); o.off.resize(3 * nl + 1);
    int64_t motif_bases = 0, units_at = 0;
    for (size_t l = 0; l < nl; l++) {
        const int64_t U = seq_off[3 * l + 2] - seq_off[3 * l + 1];
        motif_bases += U;
        o.mot_off[l + 1] = motif_bases;
        if (!la_length_ok(false, U)) o.first_bad_length = std::min(o.first_bad_length, la_key(0, (int64_t)l, -1));
        if (U > MDP_MAX_U && o.first_long_motif < 0) o.first_long_motif = (int64_t)l;
        o.ulen[l] = (int32_t)std::min<int64_t>(U, INT32_MAX);
        const int64_t u = std::min<int64_t>(U, MTRC_MAX_PERIOD);
        o.unit_off[2 * l] = (int32_t)units_at; o.unit_off[2 * l + 1] = (int32_t)(units_at + u); units_at += 2 * u;
        for (int side = 0; side < 2; side++) {
            const int64_t m = seq_off[3 * l + 2 * (size_t)side + 1] - seq_off[3 * l + 2 * (size_t)side];
            if (!la_length_ok(true, m)) o.first_bad_length = std::min(o.first_bad_length, la_key(1, 2 * (int64_t)l + side, -1));
            const int32_t mm = (int32_t)std::min<int64_t>(m, INT32_MAX);
            o.plen[4 * l + (size_t)side] = mm; o.plen[4 * l + 2 + (size_t)side] = mm;
            (m <= 32 ? o.n_short : o.n_long) += 2;
        }
        for (int k = 0; k < 3; k++) o.off[3 * l + (size_t)k] = seq_off[3 * l + (size_t)k] - seq_off[0];
    }
    o.unit_off[2 * nl] = (int32_t)units_at;
    o.off[3 * nl] = seq_off[3 * nl] - seq_off[0];
}
// the smallest key of a byte that is none of ACGT in a sequence of legal length, by a walk in the checks' order (what mtr_k_catb_check finds)
inline unsigned long long la_first_bad_letter(const char *seqs, const int64_t *seq_off, int32_t n_loci)
{
    for (int pass = 0; pass < 2; pass++)
        for (int64_t i = 0; i < (pass ? 2 : 1) * (int64_t)n_loci; i++) {
            const unsigned long long key = la_key(pass, i, -1);
            const size_t k = la_key_seq(key);
            const int64_t len = seq_off[k + 1] - seq_off[k], t = la_seq_check(pass, seqs + seq_off[k], len);
            if (t >= 0 && t < len) return key + (unsigned long long)(t + 1);
        }
    return LA_NO_KEY;
}
// the catalogue calls' checks of the seeds, from the flanks' lengths: seed_len, then the first flank too short for its seeds
inline bool la_check_seeds(const std::vector<int32_t> &plen, int32_t n_loci, int32_t max_flank_dist, int32_t seed_len, std::string &err)
{
    if (seed_len < SI_MIN_Q || seed_len > SI_MAX_Q) return la_refuse(err, "seed_len = " + std::to_string(seed_len) + " outside " + std::to_string(SI_MIN_Q) + ".." + std::to_string(SI_MAX_Q));
    const int64_t need = ((int64_t)max_flank_dist + 1) * seed_len;
    for (size_t s = 0; s < 2 * (size_t)n_loci; s++)
        if (plen[4 * (s / 2) + s % 2] < need)
            return la_refuse(err, la_flank_name((int64_t)(s / 2), (int)(s % 2)) + ": " + std::to_string(plen[4 * (s / 2) + s % 2]) + " bases are fewer than (max_flank_dist + 1) * seed_len = " + std::to_string(need));
    return true;
}
inline bool la_check_flank_dist(int32_t max_flank_dist, std::string &err) { return max_flank_dist >= 0 || la_refuse(err, "max_flank_dist = " + std::to_string(max_flank_dist) + ": at least 0"); }
// the limits a batch of n_reads reads sets: the motif search's hits, the genotype's pairs
inline bool la_check_hits(int64_t n_reads, int64_t n_motifs, std::string &err) { return n_reads * n_motifs <= (int64_t)INT32_MAX || la_refuse(err, std::to_string(n_reads) + " reads x " + std::to_string(n_motifs) + " motifs are more than 2^31 - 1 hits"); }
inline bool la_check_pairs(int64_t n_reads, int64_t n_loci, std::string &err) { return 2 * n_reads * n_loci <= (int64_t)INT32_MAX || la_refuse(err, std::to_string(n_reads) + " reads x " + std::to_string(n_loci) + " loci in two orientations are more than 2^31 - 1 pairs"); }
// The genotype's checks of its arguments over a batch of n_reads > 0 reads, in its order, up to the row limit: the offsets, the scores, the motifs'
// total, every motif's length and letters, the motif search's limit of hits, every flank's length and letters, max_flank_dist, the pairs.  The
// first refused length (la_lengths) and the first refused letter (la_first_bad_letter) are keys in that order: the smaller one is the refusal.
inline bool la_check_genotype(int64_t n_reads, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist, int32_t gain, int32_t mismatch, int32_t indel,
                              LociLengths &L, std::string &err)
{
    if (!la_check_offsets(seqs, seq_off, n_loci, err) || !la_check_scores(gain, mismatch, indel, err)) return false;
    la_lengths(seq_off, n_loci, L);
    if (!la_check_motif_total(n_loci, L.mot_off[(size_t)n_loci], err)) return false;
    const unsigned long long bad = std::min(L.first_bad_length, la_first_bad_letter(seqs, seq_off, n_loci));
    if (bad != LA_NO_KEY && !la_key_is_flank(bad)) { la_key_refusal(bad, seqs, seq_off, err); return false; }
    if (!la_check_hits(n_reads, n_loci, err)) return false;
    if (bad != LA_NO_KEY) { la_key_refusal(bad, seqs, seq_off, err); return false; }
    return la_check_flank_dist(max_flank_dist, err) && la_check_pairs(n_reads, n_loci, err);
}

// ---- the codes of checked text ----
inline std::vector<uint8_t> la_codes(const char *s, int64_t len)
{
    std::vector<uint8_t> c((size_t)len);
    for (int64_t t = 0; t < len; t++) c[(size_t)t] = (uint8_t)(cb_base_code(s[t]) & 3);
    return c;
}
inline std::vector<uint8_t> revcomp_codes(const std::vector<uint8_t> &c)
{
    std::vector<uint8_t> r(c.size());
    for (size_t t = 0; t < c.size(); t++) r[t] = (uint8_t)(3 - c[c.size() - 1 - t]);
    return r;
}
// the four flank patterns of every locus (A, B, rc A, rc B) as codes
inline void la_flank_patterns(const char *seqs, const int64_t *seq_off, int32_t n_loci, std::vector<std::vector<uint8_t>> &pat)
{
    pat.assign((size_t)n_loci * 4, std::vector<uint8_t>());
    for (size_t l = 0; l < (size_t)n_loci; l++)
        for (size_t side = 0; side < 2; side++) {
            pat[4 * l + side] = la_codes(seqs + seq_off[3 * l + 2 * side], seq_off[3 * l + 2 * side + 1] - seq_off[3 * l + 2 * side]);
            pat[4 * l + 2 + side] = revcomp_codes(pat[4 * l + side]);
        }
}
// the slots (slot = motif * ns + strand): codes 0..3 of the motif, then of its reverse complement; for U <= MDP_MAX_U the 2-bit form as well
inline void motif_slots(const char *motifs, const int64_t *motif_off, int32_t n_motifs, int ns, std::vector<uint8_t> &units, std::vector<int32_t> &unit_off,
                        std::vector<uint64_t> &bits)
{
    const size_t S = (size_t)n_motifs * (size_t)ns;
    units.clear(); unit_off.assign(S + 1, 0); bits.assign(S, 0);
    for (int32_t m = 0; m < n_motifs; m++) {
        const int U = (int)(motif_off[m + 1] - motif_off[m]);
        for (int s = 0; s < ns; s++) {
            const size_t at = units.size();
            units.resize(at + (size_t)U);
            cb_motif_codes(motifs + motif_off[m], U, s, units.data() + at);
            unit_off[(size_t)(m * ns + s) + 1] = (int32_t)units.size();
            bits[(size_t)(m * ns + s)] = mdp_motif_bits(units.data() + at, U);
        }
    }
}
// the variants of every locus: M, reversed M, rc M, reversed rc M at bits[4 * locus ..], as motif_ext takes them, and the motifs' lengths
inline void partial_variants(const std::string &mot, const std::vector<int64_t> &mot_off, int32_t n_loci, std::vector<uint64_t> &bits, std::vector<int32_t> &ulen)
{
    bits.assign((size_t)n_loci * 4, 0); ulen.assign((size_t)n_loci, 0);
    for (int32_t l = 0; l < n_loci; l++) {
        const int U = (int)(mot_off[(size_t)l + 1] - mot_off[(size_t)l]);
        const std::vector<uint8_t> c = la_codes(mot.data() + mot_off[(size_t)l], U), rc = revcomp_codes(c), rev(c.rbegin(), c.rend()), rrc(rc.rbegin(), rc.rend());
        const std::vector<uint8_t> *four[4] = { &c, &rev, &rc, &rrc };
        for (int k = 0; k < 4; k++) bits[(size_t)l * 4 + (size_t)k] = mdp_motif_bits(four[k]->data(), U);
        ulen[(size_t)l] = U;
    }
}
