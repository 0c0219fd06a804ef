// window_structure_args_check.cpp — the checks of the window-structure call's host arguments (mtr_amd/csrc/window_structure_args.h), as a program
// of its own (the form a sanitizer build runs), against a plain sequential model written here from the order include/mtr_hip.h documents: one
// check after the other, each class of refusal over all structures before the next, stopping at the first.  The header finds the same refusal as
// the smallest key of one walk over the structures, so status and words must agree for every set, whichever class comes first.  Accepted
// structures' lane forms (WsStruct) are held to a construction column by column.
#include "../mtr_amd/csrc/window_structure_args.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng >> 4; }      // xorshift32
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static long g_checks = 0;
static void same(const std::string &what, const std::string &got, const std::string &want)
{
    g_checks++;
    if (got != want) { fprintf(stderr, "FAIL: %s\n  header: %s\n  model:  %s\n", what.c_str(), got.c_str(), want.c_str()); exit(1); }
}

struct Case {
    std::string name, text; std::vector<int64_t> moff; std::vector<int32_t> soff;
    bool null_text = false, null_moff = false, null_soff = false, columns_null = false;
    int32_t n = 0, gain = 1, mismatch = 1, indel = 1; int64_t n_windows = 3, n_bases = 40;
};
static Case make_case(const std::string &name, const std::vector<std::vector<std::string>> &structs, int pad = 0)
{
    Case c; c.name = name; c.text = std::string((size_t)pad, '#'); c.moff.push_back(pad); c.soff.push_back(0); c.n = (int32_t)structs.size();
    for (const auto &st : structs) { for (const auto &m : st) { c.text += m; c.moff.push_back((int64_t)c.text.size()); } c.soff.push_back((int32_t)c.moff.size() - 1); }
    return c;
}

// ---- the model: "" when nothing is refused ----
static std::string model(const Case &c)
{
    if (c.null_text || c.null_moff || c.null_soff) return "motifs, motif_off or struct_off is NULL";
    if (c.columns_null) return "a device column or dst or one of its columns is NULL";
    if (c.n < 1 || c.n > (1 << 24)) return "n_structs = " + std::to_string(c.n) + " outside 1..2^24";
    if (c.n_windows < 0 || c.n_windows > 2147483647ll) return "n_windows = " + std::to_string(c.n_windows) + " outside 0..2^31 - 1";
    if (c.n_bases < 0) return "n_bases = " + std::to_string(c.n_bases) + " is negative";
    if (c.gain < 1 || c.gain > 5) return "gain = " + std::to_string(c.gain) + " outside 1..5";
    if (c.mismatch < 1 || c.mismatch > 3) return "mismatch = " + std::to_string(c.mismatch) + " outside 1..3";
    if (c.indel < 1 || c.indel > 3) return "indel = " + std::to_string(c.indel) + " outside 1..3";
    if (c.soff[0] < 0) return "struct_off[0] = " + std::to_string(c.soff[0]) + " is negative";
    for (int k = 0; k < c.n; k++) if (c.soff[(size_t)k + 1] < c.soff[(size_t)k]) return "struct_off decreases at structure " + std::to_string(k);
    for (int m = c.soff[0]; m < c.soff[(size_t)c.n]; m++) if (c.moff[(size_t)m + 1] < c.moff[(size_t)m]) return "motif_off decreases at motif " + std::to_string(m);
    const auto S = [&](int k) { return c.soff[(size_t)k + 1] - c.soff[(size_t)k]; };
    const auto U = [&](int k, int s) { return c.moff[(size_t)c.soff[(size_t)k] + (size_t)s + 1] - c.moff[(size_t)c.soff[(size_t)k] + (size_t)s]; };
    for (int k = 0; k < c.n; k++) if (S(k) < 1 || S(k) > 4) return "structure " + std::to_string(k) + ": " + std::to_string(S(k)) + " motifs outside 1..4";
    for (int k = 0; k < c.n; k++) for (int s = 0; s < S(k); s++) if (U(k, s) == 0) return "structure " + std::to_string(k) + ", motif " + std::to_string(s) + ": length 0";
    for (int k = 0; k < c.n; k++) {
        int64_t W = 0;
        for (int s = 0; s < S(k); s++) W += U(k, s);
        if (W > (S(k) <= 2 ? 32 : 16))
            return "structure " + std::to_string(k) + ": " + std::to_string(S(k)) + " motifs of " + std::to_string(W) + " bases in all; at most 32 bases for up to 2 motifs, 16 for up to 4";
    }
    for (int k = 0; k < c.n; k++) for (int s = 0; s < S(k); s++) for (int64_t t = 0; t < U(k, s); t++) {
        const char ch = c.text[(size_t)(c.moff[(size_t)c.soff[(size_t)k] + (size_t)s] + t)];
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T')
            return "structure " + std::to_string(k) + ", motif " + std::to_string(s) + ": byte " + std::to_string((int)(unsigned char)ch) + " at " + std::to_string(t) + " is none of ACGT";
    }
    return "";
}

static void check(const Case &c)
{
    std::string err;
    const bool ok = wsa_check(c.null_text ? nullptr : c.text.data(), c.null_moff ? nullptr : c.moff.data(), c.null_soff ? nullptr : c.soff.data(), c.n, c.columns_null, c.n_windows,
                              c.n_bases, c.gain, c.mismatch, c.indel, err);
    const std::string want = model(c);
    same(c.name + ": the verdict", ok ? "accepted" : "refused", want.empty() ? "accepted" : "refused");
    if (!ok) { same(c.name + ": the words", err, want); return; }
    for (int k = 0; k < c.n; k++) {                               // the lane form, column by column
        const WsStruct st = wsa_struct(c.text.data(), c.moff.data(), c.soff.data(), k);
        std::string got, built;
        int col = 0;
        for (int s = c.soff[(size_t)k]; s < c.soff[(size_t)k + 1]; s++)
            for (int64_t t = c.moff[(size_t)s]; t < c.moff[(size_t)s + 1]; t++, col++) {
                built += c.text[(size_t)t]; built += (char)('0' + (s - c.soff[(size_t)k])); built += t == c.moff[(size_t)s] ? 'f' : '-'; built += t == c.moff[(size_t)s + 1] - 1 ? 'l' : '-';
                got += "ACGT"[(st.mot >> (2 * col)) & 3]; got += (char)('0' + ((st.seg >> (2 * col)) & 3)); got += (st.first >> col) & 1 ? 'f' : '-'; got += (st.last >> col) & 1 ? 'l' : '-';
            }
        same(c.name + ": structure " + std::to_string(k) + "'s columns", got + " W" + std::to_string(st.W) + " S" + std::to_string(st.S),
             built + " W" + std::to_string(col) + " S" + std::to_string(c.soff[(size_t)k + 1] - c.soff[(size_t)k]));
        if (col < 32 && ((st.first | st.last) >> col)) same(c.name + ": bits beyond W", "set", "clear");
    }
}

int main(int argc, char **argv)
{
    const int random_sets = argc > 1 ? atoi(argv[1]) : 400;
    std::vector<Case> named;
    named.push_back(make_case("plain", { { "CAG" }, { "CAG", "CAACAG", "CCG" }, { "A" } }));
    named.push_back(make_case("padded text", { { "CAGG", "CAGA", "CA" }, { "ACGT", "ACGT", "ACGT", "ACGT" } }, 5));
    named.push_back(make_case("at the limits", { { std::string(32, 'A') }, { std::string(16, 'C'), std::string(16, 'G') }, { std::string(13, 'T'), "A", "C", "G" } }));
    named.push_back(make_case("33 narrow", { { "CAG" }, { std::string(16, 'C'), std::string(17, 'G') } }));
    named.push_back(make_case("17 wide", { { std::string(15, 'C'), "A", "G" } }));
    named.push_back(make_case("five motifs after a bad byte", { { "CNG" }, { "A", "C", "G", "T", "A" } }));
    named.push_back(make_case("no motifs", { { "CAG" }, {} }));
    named.push_back(make_case("an empty motif before a long structure", { { std::string(40, 'A') }, { "A", "" } }));
    named.push_back(make_case("a bad byte in the last motif", { { "CAG", "CCG" }, { "A", "C", "G", "Tx" } }));
    { Case c = make_case("NULL offsets", { { "CAG" } }); c.null_moff = true; named.push_back(c); }
    { Case c = make_case("NULL columns before the counts", { { "CAG" } }); c.columns_null = true; c.n = 0; named.push_back(c); }
    { Case c = make_case("no structures", { { "CAG" } }); c.n = 0; named.push_back(c); }
    { Case c = make_case("too many windows before the scores", { { "CAG" } }); c.n_windows = 1ll << 31; c.gain = 9; named.push_back(c); }
    { Case c = make_case("scores before the offsets", { { "CAG" }, { "CCG" } }); c.indel = 0; c.moff[1] = 9; named.push_back(c); }
    { Case c = make_case("struct_off decreases", { { "CAG" }, { "CCG" }, { "A" } }); c.soff[2] = 0; named.push_back(c); }
    { Case c = make_case("motif_off decreases", { { "CAG", "CCG" }, { "A" } }); c.moff[2] = 1; named.push_back(c); }
    for (const Case &c : named) check(c);
    for (int t = 0; t < random_sets; t++) {
        std::vector<std::vector<std::string>> structs;
        for (int k = rnd_in(1, 6); k > 0; k--) {
            std::vector<std::string> st;
            const int S = rnd_in(0, 19) == 0 ? rnd_in(0, 6) : rnd_in(1, 4);
            for (int s = 0; s < S; s++) {
                std::string m;
                for (int u = rnd_in(0, 14) == 0 ? 0 : rnd_in(1, S <= 2 ? 18 : 6); u > 0; u--) m += rnd_in(0, 39) == 0 ? "NnX acgt"[rnd_in(0, 7)] : "ACGT"[rnd_in(0, 3)];
                st.push_back(m);
            }
            structs.push_back(st);
        }
        Case c = make_case("random " + std::to_string(t), structs, rnd_in(0, 3));
        if (rnd_in(0, 29) == 0) c.mismatch = rnd_in(0, 4);
        check(c);
    }
    printf("ok: %zu named cases, %d random sets of structures, %ld checks\n", named.size(), random_sets, g_checks);
    return 0;
}
