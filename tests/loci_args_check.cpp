// loci_args_check.cpp — what the text and the lengths of a set of loci decide (mtr_amd/csrc/loci_args.h), as a program of its own (the form a
// sanitizer build runs), against a plain sequential model of the checks written here from the order the genotype calls and mtr_catalog_create
// document (include/mtr_hip.h): one walk, sequence by sequence, that stops at the first refusal and knows nothing of keys.  The header finds
// the same refusal as the smallest of two keys - the first refused length of its pass over the lengths, the first refused letter of a scan
// that skips refused lengths (on the device for mtr_catalog_create) - so status and words must agree for every catalogue, whichever of the two
// comes first.  Accepted catalogues' arrays are held to brute force: the lengths' arrays, the flanks' codes, the variants' bits, and the
// two-strand motif slots against "reverse-complement the text, then lay out one strand".
#include "../mtr_amd/csrc/loci_args.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng >> 4; }      // xorshift32
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static long g_checks = 0;
static void fail(const std::string &what, const std::string &a, const std::string &b)
{
    fprintf(stderr, "FAIL: %s\n  header: %s\n  model:  %s\n", what.c_str(), a.c_str(), b.c_str());
    exit(1);
}
static void same(const std::string &what, const std::string &got, const std::string &want) { g_checks++; if (got != want) fail(what, got, want); }
template <typename T> static void same_v(const std::string &what, const std::vector<T> &got, const std::vector<T> &want)
{
    g_checks++;
    if (got != want) fail(what, "a vector of " + std::to_string(got.size()), "differs from the brute-force one of " + std::to_string(want.size()));
}

static int brute_code(char c) { for (int k = 0; k < 4; k++) if (c == "ACGT"[k]) return k; return -1; }

// a set of loci and a call's arguments; off may be NULL, and n is given apart from the offsets' count (n_loci 0)
struct Case {
    std::string name, text; std::vector<int64_t> off; bool null_off = false;
    int32_t n = 0, K = 1, q = 8, gain = 1, mismatch = 1, indel = 1; int64_t n_reads = 5;
};
static Case make_case(const std::string &name, const std::vector<std::vector<std::string>> &loci, int pad = 0)
{
    Case c; c.name = name; c.text = std::string((size_t)pad, '#'); c.off.push_back(pad); c.n = (int32_t)loci.size();
    for (const auto &l : loci) for (const auto &s : l) { c.text += s; c.off.push_back((int64_t)c.text.size()); }
    return c;
}

// ---- the model: the checks one after the other, "" when nothing is refused ----
// create: mtr_catalog_create's (no batch, no scores, no limits of a batch); otherwise a text-taking catalogue call's, the DP's size apart
static std::string seq_refusal(const std::string &what, const char *s, int64_t len, int64_t max_len)
{
    if (len < 1 || len > max_len) return what + ": length " + std::to_string(len) + " outside 1.." + std::to_string(max_len);
    for (int64_t t = 0; t < len; t++)
        if (s[t] != 'A' && s[t] != 'C' && s[t] != 'G' && s[t] != 'T') return what + ": byte " + std::to_string((int)(unsigned char)s[t]) + " at " + std::to_string(t) + " is none of ACGT";
    return "";
}
static std::string flank_name(int l, int side) { return "locus " + std::to_string(l) + ", " + (side ? "right" : "left") + " flank"; }
static std::string model(const Case &c, bool create)
{
    const char *seqs = c.text.data(); const int64_t *off = c.null_off ? nullptr : c.off.data();
    const int n = c.n;
    if (!create && c.n_reads <= 0) return "no batch uploaded";
    if (n <= 0) return "n_loci = " + std::to_string(n) + ": at least one locus is needed";
    if (!off) return "seqs or seq_off is NULL";
    if (n > INT32_MAX / 4) return "more than 2^29 - 1 loci";
    for (int k = 0; k < 3 * n; k++) if (off[k + 1] < off[k]) return "seq_off decreases at locus " + std::to_string(k / 3) + " (sequence " + std::to_string(k % 3) + ")";
    if (!create) {
        if (c.gain < 1 || c.gain > 5) return "gain = " + std::to_string(c.gain) + " outside 1..5";
        if (c.mismatch < 1 || c.mismatch > 3) return "mismatch = " + std::to_string(c.mismatch) + " outside 1..3";
        if (c.indel < 1 || c.indel > 3) return "indel = " + std::to_string(c.indel) + " outside 1..3";
    }
    int64_t motif_bases = 0;
    for (int l = 0; l < n; l++) motif_bases += off[3 * l + 2] - off[3 * l + 1];
    if (motif_bases > INT32_MAX / 2) return "more than 2^30 - 1 motifs or motif bases";      // (never with texts of this size: here for the order's sake)
    for (int l = 0; l < n; l++) { const std::string r = seq_refusal("motif " + std::to_string(l), seqs + off[3 * l + 1], off[3 * l + 2] - off[3 * l + 1], 499); if (!r.empty()) return r; }
    if (!create && c.n_reads * n > (int64_t)INT32_MAX) return std::to_string(c.n_reads) + " reads x " + std::to_string(n) + " motifs are more than 2^31 - 1 hits";
    for (int l = 0; l < n; l++)
        for (int side = 0; side < 2; side++) {
            const std::string r = seq_refusal(flank_name(l, side), seqs + off[3 * l + 2 * side], off[3 * l + 2 * side + 1] - off[3 * l + 2 * side], 64);
            if (!r.empty()) return r;
        }
    if (c.K < 0) return "max_flank_dist = " + std::to_string(c.K) + ": at least 0";
    if (!create && 2 * c.n_reads * n > (int64_t)INT32_MAX) return std::to_string(c.n_reads) + " reads x " + std::to_string(n) + " loci in two orientations are more than 2^31 - 1 pairs";
    if (c.q < 8 || c.q > 16) return "seed_len = " + std::to_string(c.q) + " outside 8..16";
    const int64_t need = ((int64_t)c.K + 1) * c.q;
    for (int l = 0; l < n; l++)
        for (int side = 0; side < 2; side++) {
            const int64_t m = off[3 * l + 2 * side + 1] - off[3 * l + 2 * side];
            if (m < need) return flank_name(l, side) + ": " + std::to_string(m) + " bases are fewer than (max_flank_dist + 1) * seed_len = " + std::to_string(need);
        }
    return "";
}

// ---- the header, called as the entry points call it ----
static std::string header_text_call(const Case &c, LociLengths &L)
{
    std::string err;
    const int64_t *off = c.null_off ? nullptr : c.off.data();
    if (c.n_reads <= 0) return "no batch uploaded";
    if (!la_check_genotype(c.n_reads, c.text.data(), off, c.n, c.K, c.gain, c.mismatch, c.indel, L, err)) return err;
    if (!la_check_seeds(L.plen, c.n, c.K, c.q, err)) return err;
    return "";
}
static std::string header_create(const Case &c, LociLengths &L)
{
    std::string err;
    const char *seqs = c.text.data(); const int64_t *off = c.null_off ? nullptr : c.off.data();
    if (!la_check_offsets(seqs, off, c.n, err)) return err;
    la_lengths(off, c.n, L);
    if (!la_check_motif_total(c.n, L.mot_off[(size_t)c.n], err)) return err;
    const unsigned long long bad = std::min(L.first_bad_length, la_first_bad_letter(seqs, off, c.n));      // (the device's part: mtr_k_catb_check)
    if (bad != LA_NO_KEY) { if (!la_key_refusal(bad, seqs, off, err)) return "a key that names no byte"; return err; }
    if (!la_check_flank_dist(c.K, err) || !la_check_seeds(L.plen, c.n, c.K, c.q, err)) return err;
    return "";
}

// ---- accepted loci: the arrays against brute force ----
static std::vector<uint8_t> brute_codes(const std::string &s) { std::vector<uint8_t> c; for (char ch : s) c.push_back((uint8_t)brute_code(ch)); return c; }
static std::string brute_revcomp_text(const std::string &s) { std::string r; for (size_t t = s.size(); t-- > 0;) r += "ACGT"[3 - brute_code(s[t])]; return r; }
static uint64_t brute_bits(const std::vector<uint8_t> &c) { uint64_t m = 0; for (size_t j = 0; j < c.size() && j < 32; j++) m |= (uint64_t)c[j] << (2 * j); return m; }

static void check_accepted(const Case &c, const LociLengths &L)
{
    const size_t nl = (size_t)c.n;
    const int64_t *off = c.off.data();
    std::vector<std::string> A(nl), M(nl), B(nl);
    for (size_t l = 0; l < nl; l++) {
        A[l] = c.text.substr((size_t)off[3 * l], (size_t)(off[3 * l + 1] - off[3 * l])); M[l] = c.text.substr((size_t)off[3 * l + 1], (size_t)(off[3 * l + 2] - off[3 * l + 1]));
        B[l] = c.text.substr((size_t)off[3 * l + 2], (size_t)(off[3 * l + 3] - off[3 * l + 2]));
    }
    // the lengths' arrays
    std::vector<int64_t> mot_off(1, 0), reb; std::vector<int32_t> unit_off(1, 0), plen, ulen;
    int64_t n_short = 0, n_long = 0, first_long = -1;
    std::string mot;
    for (size_t l = 0; l < nl; l++) {
        mot += M[l]; mot_off.push_back((int64_t)mot.size());
        for (int s = 0; s < 2; s++) unit_off.push_back(unit_off.back() + (int32_t)M[l].size());
        const int32_t four[4] = { (int32_t)A[l].size(), (int32_t)B[l].size(), (int32_t)A[l].size(), (int32_t)B[l].size() };
        for (int j = 0; j < 4; j++) { plen.push_back(four[j]); (four[j] <= 32 ? n_short : n_long)++; }
        ulen.push_back((int32_t)M[l].size());
        if (M[l].size() > 32 && first_long < 0) first_long = (int64_t)l;
    }
    for (int64_t o : c.off) reb.push_back(o - c.off[0]);
    same_v(c.name + ": mot_off", L.mot_off, mot_off); same_v(c.name + ": unit_off", L.unit_off, unit_off); same_v(c.name + ": plen", L.plen, plen);
    same_v(c.name + ": ulen", L.ulen, ulen); same_v(c.name + ": rebased offsets", L.off, reb);
    same(c.name + ": n_short, n_long, first_long_motif", std::to_string(L.n_short) + " " + std::to_string(L.n_long) + " " + std::to_string(L.first_long_motif),
         std::to_string(n_short) + " " + std::to_string(n_long) + " " + std::to_string(first_long));
    same(c.name + ": first_bad_length", std::to_string(L.first_bad_length), std::to_string(LA_NO_KEY));
    // the flanks' codes: A, B, rc A, rc B
    std::vector<std::vector<uint8_t>> pat;
    la_flank_patterns(c.text.data(), off, c.n, pat);
    for (size_t l = 0; l < nl; l++) {
        const std::string four[4] = { A[l], B[l], brute_revcomp_text(A[l]), brute_revcomp_text(B[l]) };
        for (size_t j = 0; j < 4; j++) same_v(c.name + ": flank pattern", pat[4 * l + j], brute_codes(four[j]));
    }
    // the two-strand slots against: reverse-complement the text, lay out one strand of 2 * n motifs
    std::vector<uint8_t> units, want_units; std::vector<int32_t> uoff, want_uoff(1, 0); std::vector<uint64_t> bits, want_bits;
    motif_slots(mot.data(), mot_off.data(), c.n, 2, units, uoff, bits);
    for (size_t l = 0; l < nl; l++)
        for (const std::string &s : { M[l], brute_revcomp_text(M[l]) }) {
            const std::vector<uint8_t> codes = brute_codes(s);
            want_units.insert(want_units.end(), codes.begin(), codes.end()); want_uoff.push_back((int32_t)want_units.size()); want_bits.push_back(brute_bits(codes));
        }
    same_v(c.name + ": slots' units", units, want_units); same_v(c.name + ": slots' offsets", uoff, want_uoff); same_v(c.name + ": slots' bits", bits, want_bits);
    same_v(c.name + ": slots' offsets are the lengths' unit_off", uoff, L.unit_off);
    // the variants: M, reversed M, rc M, reversed rc M
    std::vector<uint64_t> vbits, want_v; std::vector<int32_t> vlen;
    partial_variants(mot, mot_off, c.n, vbits, vlen);
    for (size_t l = 0; l < nl; l++) {
        const std::string rc = brute_revcomp_text(M[l]);
        for (const std::string &s : { M[l], std::string(M[l].rbegin(), M[l].rend()), rc, std::string(rc.rbegin(), rc.rend()) }) want_v.push_back(brute_bits(brute_codes(s)));
    }
    same_v(c.name + ": variants' bits", vbits, want_v); same_v(c.name + ": variants' lengths", vlen, ulen);
}

static long g_accepted = 0, g_refused_len = 0, g_refused_byte = 0;
static void check_case(const Case &c)
{
    for (int create = 0; create < 2; create++) {
        LociLengths L;
        const std::string got = create ? header_create(c, L) : header_text_call(c, L), want = model(c, create);
        same(c.name + (create ? " (create)" : " (text-taking)"), got, want);
        if (got.empty() && create) { g_accepted++; check_accepted(c, L); }
        if (create && got.find(": length ") != std::string::npos) g_refused_len++;
        if (create && got.find(": byte ") != std::string::npos) g_refused_byte++;
    }
}

// ---- the named cases of tests/test_gpu_catalog_prepared.py's BAD ----
static void check_named()
{
    const std::string A = "ACGTACGTACGGTCAT", B = "TTGACCGATAGGCTAA", long_motif = [] { std::string s; for (int k = 0; k < 100; k++) s += "ACGTC"; return s; }(),
                      f65 = [] { std::string s; for (int k = 0; k < 16; k++) s += "ACGT"; return s + "A"; }();
    const std::vector<std::string> OK = { A, "CAG", B };
    std::vector<Case> v;
    v.push_back(make_case("a bad letter in a motif", { OK, { A, "CNG", B } }));
    v.push_back(make_case("a bad letter in a flank", { OK, { A, "CAG", B.substr(0, 7) + "x" + B.substr(8) } }));
    v.push_back(make_case("a bad flank letter before a later bad motif length", { { A.substr(0, 3) + "N" + A.substr(4), "CAG", B }, { A, "", B } }));
    v.push_back(make_case("a bad motif letter at a later locus against a bad flank length at an earlier one", { { A, "CAG", "" }, OK, { A, "CNG", B } }));
    v.push_back(make_case("a bad flank letter against a later bad flank length", { { A, "CAG", B.substr(0, 5) + "n" + B.substr(6) }, { A, "CAG", f65 } }));
    v.push_back(make_case("a bad flank length against a later bad flank letter", { { "", "CAG", B }, { A.substr(0, 2) + "N" + A.substr(3), "CAG", B } }));
    v.push_back(make_case("a bad flank letter in the right flank against a bad length of the same locus' left flank", { OK, { "", "CAG", "NCGT" + B.substr(4) } }));
    v.push_back(make_case("a bad motif length against an earlier bad motif letter", { { A, "CAGN", B }, { A, "", B } }));
    v.push_back(make_case("a bad motif letter against an earlier bad motif length", { { A, long_motif, B }, { A, "CxG", B } }));
    v.push_back(make_case("a flank of 0 bases", { { A, "CAG", "" } }));
    v.push_back(make_case("a flank of 65 bases", { { f65, "CAG", B } }));
    v.push_back(make_case("a motif of 500 bases", { { A, long_motif, B } }));
    { Case c = make_case("a decreasing seq_off", { OK }); c.off = { 0, 16, 12, 35 }; v.push_back(c); }
    v.push_back(make_case("a short flank for (K, q)", { OK, { A, "CAG", B.substr(0, 15) } }));
    { Case c = make_case("K too large for the flanks", { OK }); c.K = 2; v.push_back(c); }
    { Case c = make_case("seed_len 7", { OK }); c.q = 7; v.push_back(c); }
    { Case c = make_case("seed_len 17", { OK }); c.q = 17; v.push_back(c); }
    { Case c = make_case("n_loci 0", { OK }); c.n = 0; v.push_back(c); }
    { Case c = make_case("negative K", { OK }); c.K = -1; v.push_back(c); }
    if (v.size() != 19) fail("the named cases", std::to_string(v.size()), "19");
    for (const Case &c : v) {
        check_case(c);
        if (model(c, true).empty()) fail(c.name, "accepted", "a refusal");
    }
    // beside them: what only arguments can show
    { Case c = make_case("NULL offsets", { OK }); c.null_off = true; check_case(c); }
    { Case c = make_case("no batch", { OK }); c.n_reads = 0; check_case(c); }
    { Case c = make_case("more hits than 2^31 - 1", { OK, OK }); c.n_reads = INT32_MAX; check_case(c); }
    { Case c = make_case("more pairs than 2^31 - 1", { OK }); c.n_reads = ((int64_t)1 << 30) + 1; check_case(c); }
    { Case c = make_case("the hits' limit before a bad flank", { OK, { A, "CAG", "" } }); c.n_reads = INT32_MAX; check_case(c); }
    { Case c = make_case("accepted, from a nonzero first offset", { OK, { B, "ACGTACGTACGTACGTACGTACGTACGTACGTA", A } }, 7); check_case(c); }
    std::string err = "kept";
    const Case c = make_case("a key past its sequence", { OK });
    if (la_key_refusal(la_key(0, 0, 3), c.text.data(), c.off.data(), err) || err != "kept") fail("a key past its sequence", err, "refused, err kept");
}

// ---- random catalogues: 1..4 loci, flanks of 0..66 and motifs of 0..40 bases (one of 500 now and then), letters of ACGTNacgtx ----
static std::string rnd_seq(int len, bool clean) { std::string s((size_t)len, 'A'); for (char &ch : s) ch = clean || rnd() % 24 ? "ACGT"[rnd() & 3u] : "ACGTNacgtx"[rnd() % 10]; return s; }
static void check_random(int count)
{
    for (int k = 0; k < count; k++) {
        const int n = rnd_in(1, 4), mode = (int)(rnd() % 4);       // 0: everything at random; 1..3: legal lengths and letters mostly, so that later checks are reached
        std::vector<std::vector<std::string>> loci;
        for (int l = 0; l < n; l++) {
            const bool clean = mode != 0 && rnd() % 8 != 0;
            const int a = mode ? rnd_in(rnd() % 8 ? 16 : 0, rnd() % 8 ? 64 : 66) : rnd_in(0, 66), b = mode ? rnd_in(rnd() % 8 ? 16 : 0, rnd() % 8 ? 64 : 66) : rnd_in(0, 66);
            const int u = rnd() % 16 == 0 ? 500 : rnd_in(mode && rnd() % 8 ? 1 : 0, 40);
            loci.push_back({ rnd_seq(a, clean), rnd_seq(u, clean), rnd_seq(b, clean) });
        }
        Case c = make_case("random catalogue " + std::to_string(k), loci, (int)(rnd() % 3) * 5);
        c.K = mode ? rnd_in(rnd() % 8 ? 0 : -1, 3) : rnd_in(-1, 3); c.q = mode ? rnd_in(rnd() % 8 ? 8 : 7, rnd() % 8 ? 16 : 17) : rnd_in(7, 17);
        c.gain = mode && rnd() % 8 ? rnd_in(1, 5) : rnd_in(0, 6); c.mismatch = mode && rnd() % 8 ? rnd_in(1, 3) : rnd_in(0, 6); c.indel = mode && rnd() % 8 ? rnd_in(1, 3) : rnd_in(0, 6);
        if (mode >= 2) { c.K = rnd_in(0, 1); c.q = c.K ? 8 : rnd_in(8, 16); }      // seeds that flanks of 16 bases hold
        if (rnd() % 32 == 0) { const size_t at = 1 + rnd() % (c.off.size() - 1); c.off[at] = c.off[at - 1] - 1; }      // (every sequence still lies inside the text's buffer or is never read)
        if (rnd() % 32 == 0) c.n_reads = rnd() % 2 ? INT32_MAX : 0;
        check_case(c);
    }
}

int main(int argc, char **argv)
{
    const int count = argc > 1 ? atoi(argv[1]) : 400;
    check_named();
    check_random(count);
    if (g_accepted < count / 10 || g_refused_len < count / 20 || g_refused_byte < count / 20) {
        fprintf(stderr, "FAIL: the random catalogues are lopsided: %ld accepted, %ld refused for a length, %ld for a byte\n", g_accepted, g_refused_len, g_refused_byte);
        return 1;
    }
    printf("ok: 19 named cases, %d random catalogues (%ld accepted, %ld refused for a length, %ld for a byte), %ld comparisons\n", count, g_accepted, g_refused_len, g_refused_byte, g_checks);
    return 0;
}
