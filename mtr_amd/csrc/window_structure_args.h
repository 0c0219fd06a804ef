// window_structure_args.h — what the host arguments of the window-structure call decide (mtr_window_structure_device): the checks with their
// refusals' words, and the structures as the lanes carry them (WsStruct).  Plain C++17, nothing of HIP, in loci_args.h's way: the host side of the
// library and a host-only program (tests/window_structure_args_check.cpp) compile the same functions.
//   order       NULLs; the counts; the scores; struct_off, then motif_off, decreasing; then, each over ALL structures before the next: a structure of
//               0 or more than WS_MAX_SEGMENTS motifs, a motif of length 0, the column limit, a byte that is none of ACGT.
//   key         the place of a refusal of the last four kinds, ordered as those checks go: bits 60..61 the kind (0 the motifs' count, 1 a motif's
//               length, 2 the column limit, 3 a byte), bits 8..39 the structure, bits 6..7 the motif within it, bits 0..5 the byte within the
//               motif.  The smallest key is the refusal a sequential walk meets first.
//   refusal     every function here that checks returns true, or false with the reason in `err`; the status is the caller's (MTR_ERR_BAD_ARG).
#pragma once
#include <string>
#include <vector>

#include "loci_args.h"
#include "window_structure.h"

#define WSA_NO_KEY (~0ull)
#define WSA_MAX_STRUCTS ((int64_t)1 << 24)

inline unsigned long long wsa_key(int kind, int64_t structure, int motif, int t) { return ((unsigned long long)kind << 60) | ((unsigned long long)structure << 8) | ((unsigned long long)motif << 6) | (unsigned long long)t; }
inline int wsa_key_kind(unsigned long long key) { return (int)((key >> 60) & 3); }
inline int64_t wsa_key_struct(unsigned long long key) { return (int64_t)((key >> 8) & 0xffffffffull); }
inline int wsa_key_motif(unsigned long long key) { return (int)((key >> 6) & 3); }
inline int wsa_key_t(unsigned long long key) { return (int)(key & 63); }

// the smallest key among the structures of checked offsets (wsa_check_offsets comes first)
inline unsigned long long wsa_first_bad(const char *motifs, const int64_t *motif_off, const int32_t *struct_off, int32_t n_structs)
{
    unsigned long long bad = WSA_NO_KEY;
    for (int32_t k = 0; k < n_structs; k++) {
        const int64_t S = (int64_t)struct_off[k + 1] - struct_off[k];
        if (S < 1 || S > WS_MAX_SEGMENTS) { bad = std::min(bad, wsa_key(0, k, 0, 0)); continue; }
        int64_t W = 0; bool len0 = false;
        for (int s = 0; s < (int)S; s++) {
            const int64_t U = motif_off[struct_off[k] + s + 1] - motif_off[struct_off[k] + s];
            if (U < 1 && !len0) { bad = std::min(bad, wsa_key(1, k, s, 0)); len0 = true; }
            W += U;
        }
        if (len0) continue;
        if (!ws_limit_ok((int)S, W)) { bad = std::min(bad, wsa_key(2, k, 0, 0)); continue; }
        bool found = false;
        for (int s = 0; s < (int)S && !found; s++) {
            const int64_t at = motif_off[struct_off[k] + s], U = motif_off[struct_off[k] + s + 1] - at;
            const int64_t t = la_first_bad_byte(motifs + at, U);
            if (t < U) { bad = std::min(bad, wsa_key(3, k, s, (int)t)); found = true; }
        }
    }
    return bad;
}
inline std::string wsa_refusal(unsigned long long key, const char *motifs, const int64_t *motif_off, const int32_t *struct_off)
{
    const int64_t k = wsa_key_struct(key); const int s = wsa_key_motif(key), t = wsa_key_t(key);
    const int64_t S = (int64_t)struct_off[k + 1] - struct_off[k];
    const std::string what = "structure " + std::to_string(k);
    if (wsa_key_kind(key) == 0) return what + ": " + std::to_string(S) + " motifs outside 1.." + std::to_string(WS_MAX_SEGMENTS);
    if (wsa_key_kind(key) == 1) return what + ", motif " + std::to_string(s) + ": length 0";
    if (wsa_key_kind(key) == 2) {
        const int64_t W = motif_off[struct_off[k + 1]] - motif_off[struct_off[k]];
        return what + ": " + std::to_string(S) + " motifs of " + std::to_string(W) + " bases in all; at most " + std::to_string(WS_MAX_W_NARROW) + " bases for up to 2 motifs, " +
               std::to_string(WS_MAX_W_WIDE) + " for up to " + std::to_string(WS_MAX_SEGMENTS);
    }
    const int64_t at = motif_off[struct_off[k] + s];
    return what + ", motif " + std::to_string(s) + ": byte " + std::to_string((int)(unsigned char)motifs[at + t]) + " at " + std::to_string(t) + " is none of ACGT";
}

inline bool wsa_check_offsets(const int64_t *motif_off, const int32_t *struct_off, int32_t n_structs, std::string &err)
{
    if (struct_off[0] < 0) return la_refuse(err, "struct_off[0] = " + std::to_string(struct_off[0]) + " is negative");
    for (int32_t k = 0; k < n_structs; k++)
        if (struct_off[k + 1] < struct_off[k]) return la_refuse(err, "struct_off decreases at structure " + std::to_string(k));
    for (int32_t m = struct_off[0]; m < struct_off[n_structs]; m++)
        if (motif_off[m + 1] < motif_off[m]) return la_refuse(err, "motif_off decreases at motif " + std::to_string(m));
    return true;
}
// The call's checks of its host arguments, in its order (the pointers of the device columns and of dst: the caller's `columns_null`)
inline bool wsa_check(const char *motifs, const int64_t *motif_off, const int32_t *struct_off, int32_t n_structs, bool columns_null, int64_t n_windows, int64_t n_bases,
                      int32_t gain, int32_t mismatch, int32_t indel, std::string &err)
{
    if (!motifs || !motif_off || !struct_off) return la_refuse(err, "motifs, motif_off or struct_off is NULL");
    if (columns_null) return la_refuse(err, "a device column or dst or one of its columns is NULL");
    if (n_structs < 1 || n_structs > WSA_MAX_STRUCTS) return la_refuse(err, "n_structs = " + std::to_string(n_structs) + " outside 1..2^24");
    if (n_windows < 0 || n_windows > (int64_t)INT32_MAX) return la_refuse(err, "n_windows = " + std::to_string(n_windows) + " outside 0..2^31 - 1");
    if (n_bases < 0) return la_refuse(err, "n_bases = " + std::to_string(n_bases) + " is negative");
    if (!la_check_scores(gain, mismatch, indel, err) || !wsa_check_offsets(motif_off, struct_off, n_structs, err)) return false;
    const unsigned long long bad = wsa_first_bad(motifs, motif_off, struct_off, n_structs);
    return bad == WSA_NO_KEY || la_refuse(err, wsa_refusal(bad, motifs, motif_off, struct_off));
}

// ---- the structures of checked text ----
inline WsStruct wsa_struct(const char *motifs, const int64_t *motif_off, const int32_t *struct_off, int32_t k)
{
    WsStruct st = { 0, 0, 0, 0, 0, struct_off[k + 1] - struct_off[k] };
    int c = 0;
    for (int s = 0; s < st.S; s++) {
        const int64_t at = motif_off[struct_off[k] + s], U = motif_off[struct_off[k] + s + 1] - at;
        st.first |= 1u << c;
        for (int64_t t = 0; t < U; t++, c++) { st.mot |= (uint64_t)(cb_base_code(motifs[at + t]) & 3) << (2 * c); st.seg |= (uint64_t)s << (2 * c); }
        st.last |= 1u << (c - 1);
    }
    st.W = c;
    return st;
}
