// consensus_quality_check — the weighted vote of mtr_amd/csrc/banded_align.h (baq_walk and baq_emit, which mtr_k_cq_align and mtr_k_cq_emit run)
// built by the plain host compiler and held to a brute force written here from the header's words: the full (n + 1) x (m + 1) matrix with
// infinities outside the band, the path collected column by column, the weights, the gap weights, the `end` counters, the emission of every
// position.  Seeded alleles of 2 .. 5 members whose lengths are every pair of 0, 1, 2, 15, 16, 17, 31, 32, 33 (either side of the 16-step direction
// dword), and pairs whose bands are 127 / 128 / 129 and 255 / 256 diagonals wide, the member longer and shorter; qualities 0 .. 60; qual_cap 1,
// 10, 40 and 93; both layouts of the directions.  With qual_cap = 1 the table's first BA_TAB counters must be ba_walk's and the emission
// ba_emit's.  Prints "<cases> cases checked: ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mtr_amd/csrc/banded_align.h"

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

typedef std::vector<uint8_t> Bytes;
static const int NONE = 1 << 29;
struct Brute { std::vector<int> D, dir; int n, m; int at(int i, int j) const { return i * (m + 1) + j; } };

static Brute brute(const Bytes &W, const Bytes &B, int extra)
{
    Brute r; r.n = (int)W.size(); r.m = (int)B.size();
    const int n = r.n, m = r.m, dlo = (m - n < 0 ? m - n : 0) - extra, dhi = (m - n > 0 ? m - n : 0) + extra;
    r.D.assign((size_t)(n + 1) * (m + 1), NONE); r.dir.assign(r.D.size(), -1);
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= m; j++) {
            if (j - i < dlo || j - i > dhi) continue;
            if (i == 0 && j == 0) { r.D[0] = 0; continue; }
            const int diag = i && j && r.D[r.at(i - 1, j - 1)] < NONE ? r.D[r.at(i - 1, j - 1)] + (W[i - 1] != B[j - 1]) : NONE;
            const int up = i && r.D[r.at(i - 1, j)] < NONE ? r.D[r.at(i - 1, j)] + 1 : NONE;
            const int left = j && r.D[r.at(i, j - 1)] < NONE ? r.D[r.at(i, j - 1)] + 1 : NONE;
            int best = diag < up ? diag : up; best = best < left ? best : left;
            r.D[r.at(i, j)] = best;
            r.dir[r.at(i, j)] = diag == best ? 0 : up == best ? 1 : 2;
        }
    return r;
}

static int weight(int q, int cap) { return q < 1 ? 1 : q > cap ? cap : q; }
// the gap weight by the header's words: both neighbours where both exist, the one that exists at the ends, 1 for an empty window
static int gap(const Bytes &Q, int i, int cap)
{
    const int n = (int)Q.size();
    if (n == 0) return 1;
    const bool has_left = i >= 1, has_right = i < n;
    if (has_left && has_right) { const int a = weight(Q[(size_t)i - 1], cap), b = weight(Q[(size_t)i], cap); return a < b ? a : b; }
    return has_left ? weight(Q[(size_t)i - 1], cap) : weight(Q[(size_t)i], cap);
}

// the votes by the definition's words: first the path's cells, then per column its rows lo .. hi and how it leaves (lo, j)
static void brute_votes(const Brute &r, const Bytes &W, const Bytes &Q, int cap, std::vector<int32_t> &tab)
{
    std::vector<int> lo((size_t)r.m + 1, 1 << 30), hi((size_t)r.m + 1, -1), leave((size_t)r.m + 1, -1);
    int i = r.n, j = r.m;
    for (;;) {
        if (i < lo[(size_t)j]) lo[(size_t)j] = i;
        if (i > hi[(size_t)j]) hi[(size_t)j] = i;
        if (i == 0 && j == 0) break;
        const int d = r.dir[r.at(i, j)];
        if (d == 0) { leave[(size_t)j] = 0; i--; j--; }
        else if (d == 1) i--;
        else { leave[(size_t)j] = 2; j--; }
    }
    for (j = 0; j <= r.m; j++) {
        int32_t *t = tab.data() + (size_t)j * 25;
        const int l = lo[(size_t)j], L = hi[(size_t)j] - l;
        if (leave[(size_t)j] == 0) t[W[(size_t)l - 1]] += weight(Q[(size_t)l - 1], cap);
        if (leave[(size_t)j] == 2) t[4] += gap(Q, l, cap);
        for (int k = 0; k < L && k < 4; k++) t[5 + 4 * k + W[(size_t)(l + k)]] += weight(Q[(size_t)(l + k)], cap);
        if (L < 4) t[21 + L] += gap(Q, hi[(size_t)j], cap);
    }
}

// the emission of position j by the definition's words
static void brute_emit(const int32_t *t, int j, const Bytes &B, const Bytes &QB, int cap, std::vector<int> &sym, std::vector<int> &votes)
{
    if (j >= 1) {
        const int bb = B[(size_t)j - 1];
        int base[4]; for (int c = 0; c < 4; c++) base[c] = t[c] + (c == bb ? weight(QB[(size_t)j - 1], cap) : 0);
        int top = 0; for (int c = 0; c < 4; c++) top = base[c] > top ? base[c] : top;
        int pick = -1;
        if (base[bb] == top) pick = bb; else for (int c = 3; c >= 0; c--) if (base[c] == top) pick = c;
        if (!(t[4] > top)) { sym.push_back(pick); votes.push_back(top); }
    }
    for (int k = 0; k < 4; k++) {
        int none = gap(QB, j, cap), mx = -1, arg = 0;
        for (int L = 0; L <= k; L++) none += t[21 + L];
        for (int c = 0; c < 4; c++) if (t[5 + 4 * k + c] > mx) { mx = t[5 + 4 * k + c]; arg = c; }
        if (!(mx > none)) break;
        sym.push_back(arg); votes.push_back(mx);
    }
}

static int fail(const char *what, int n, int m, int extra, int cap, int cpl)
{
    printf("FAILED: %s (n = %d, m = %d, band_extra = %d, qual_cap = %d, cpl = %d)\n", what, n, m, extra, cap, cpl);
    return 1;
}

static Bytes random_bytes(int n, uint32_t below) { Bytes v((size_t)n); for (auto &c : v) c = (uint8_t)rnd(below); return v; }
// a member of exactly n bases related to B: B's bases with a tenth of them changed, cut or continued at random
static Bytes related(const Bytes &B, int n, uint32_t alphabet)
{
    Bytes w;
    for (size_t i = 0; i < B.size() && (int)w.size() < n; i++) { const uint32_t k = rnd(20); if (k == 0) continue; if (k == 1) w.push_back((uint8_t)rnd(alphabet)); w.push_back(k == 2 ? (uint8_t)rnd(alphabet) : B[i]); }
    if ((int)w.size() > n) w.resize((size_t)n);
    while ((int)w.size() < n) w.push_back((uint8_t)rnd(alphabet));
    return w;
}

// one allele: backbone B with qualities QB, members of the given lengths; every member's votes and then every position's emission
static int check_allele(const Bytes &B, const std::vector<int> &lens, int extra, long &cases)
{
    static const int caps[4] = { 1, 10, 40, 93 };
    const int m = (int)B.size();
    const uint32_t alphabet = 2 + rnd(3);
    const Bytes QB = random_bytes(m, 61);
    std::vector<Bytes> Ws, Qs;
    for (int n : lens) { Ws.push_back(rnd(3) ? related(B, n, alphabet) : random_bytes(n, alphabet)); Qs.push_back(random_bytes(n, 61)); }
    std::vector<int32_t> E(128), O(128);
    for (int cap : caps) {
        std::vector<int32_t> want((size_t)(m + 1) * 25, 0), got((size_t)(m + 1) * BAQ_TAB, 0), plain((size_t)(m + 1) * BA_TAB, 0);
        for (size_t w = 0; w < Ws.size(); w++) {
            const Bytes &W = Ws[w], &Q = Qs[w];
            const int n = (int)W.size();
            if (ba_skipped(n, m, extra)) return fail("a pair inside the limits is skipped", n, m, extra, cap, 0);
            const Brute r = brute(W, B, extra);
            std::vector<int32_t> one((size_t)(m + 1) * 25, 0);
            brute_votes(r, W, Q, cap, one);
            for (size_t x = 0; x < one.size(); x++) want[x] += one[x];
            const BaBand band = ba_band(n, m, extra);
            for (int cpl = ba_width(band) <= 128 ? 1 : 2; cpl <= 2; cpl++) {
                std::vector<uint32_t> dirs((size_t)ba_dir_words(n, m, cpl));
                E.assign((size_t)64 * cpl, 0); O.assign((size_t)64 * cpl, 0);
                if (ba_fill(n, m, W.data(), B.data(), band, cpl, E.data(), O.data(), dirs.data()) != r.D[r.at(n, m)]) return fail("D(n, m)", n, m, extra, cap, cpl);
                std::vector<int32_t> tab((size_t)(m + 1) * BAQ_TAB, 0);
                const uint32_t *dp = dirs.data(); const int32_t dlo = band.dlo;
                baq_walk(n, m, W.data(), Q.data(), cap, [=](int32_t i, int32_t j) { return ba_dir_at(dp, i, j, dlo, cpl); }, [&](int64_t at, int32_t v) { tab[(size_t)at] += v; });
                if (tab != one) return fail("the weighted votes", n, m, extra, cap, cpl);
                if (cpl == 2) {
                    for (size_t x = 0; x < tab.size(); x++) got[x] += tab[x];
                    if (cap == 1) ba_walk(n, m, W.data(), [=](int32_t i, int32_t j) { return ba_dir_at(dp, i, j, dlo, cpl); }, [&](int64_t at) { plain[(size_t)at]++; });
                }
                cases++;
            }
        }
        if (got != want) return fail("the votes of all members", 0, m, extra, cap, 0);
        for (int j = 0; j <= m; j++) {
            const int32_t *t = got.data() + (size_t)j * BAQ_TAB;
            std::vector<int> ws, wv, gs, gv;
            brute_emit(t, j, B, QB, cap, ws, wv);
            uint8_t sym[1 + BA_INS_SLOTS]; int32_t vt[1 + BA_INS_SLOTS];
            const int bb = j >= 1 ? B[(size_t)j - 1] : 0;
            const int em = baq_emit(t, j, bb, j >= 1 ? baq_weight(QB[(size_t)j - 1], cap) : 0, baq_gap(QB.data(), m, j, cap), sym, vt);
            if (em & 1) { gs.push_back(sym[0]); gv.push_back(vt[0]); }
            for (int k = 1; k <= em >> 1; k++) { gs.push_back(sym[k]); gv.push_back(vt[k]); }
            if (gs != ws || gv != wv) return fail("the emission", j, m, extra, cap, 0);
            if (cap == 1) {                                                  // the identity: the unweighted table and its emission
                const int32_t *p = plain.data() + (size_t)j * BA_TAB;
                for (int k = 0; k < BA_TAB; k++) if (p[k] != t[k]) return fail("qual_cap 1 is not the unweighted table", j, m, extra, cap, 0);
                uint8_t s1[1 + BA_INS_SLOTS]; int32_t v1[1 + BA_INS_SLOTS];
                if (ba_emit(p, j, bb, 1 + (int32_t)Ws.size(), s1, v1) != em) return fail("qual_cap 1 is not the unweighted emission", j, m, extra, cap, 0);
                for (int k = 0; k <= em >> 1; k++) if ((k > 0 || (em & 1)) && (s1[k] != sym[k] || v1[k] != vt[k])) return fail("qual_cap 1 is not the unweighted symbol", j, m, extra, cap, 0);
            }
            cases++;
        }
    }
    return 0;
}

int main()
{
    static const int LENGTHS[9] = { 0, 1, 2, 15, 16, 17, 31, 32, 33 };
    long cases = 0;
    for (int round = 0; round < 6; round++)
        for (int m : LENGTHS) {
            std::vector<int> lens(LENGTHS, LENGTHS + 9);
            if (round >= 3) { lens.clear(); for (uint32_t k = 0, c = 1 + rnd(4); k < c; k++) lens.push_back(LENGTHS[rnd(9)]); }     // 1 .. 4 members beside the backbone
            if (check_allele(random_bytes(m, 4), lens, round % 3 == 0 ? 16 : round % 3 == 1 ? 0 : 8, cases)) return 1;
        }
    // band_extra 16: length differences 94, 95, 96 -> 127, 128, 129 diagonals; 222, 223 -> 255, 256
    static const int DIFFS[5] = { 94, 95, 96, 222, 223 };
    for (int diff : DIFFS) {
        if (check_allele(random_bytes(40, 4), std::vector<int>{ 40 + diff, 41 }, 16, cases)) return 1;
        if (check_allele(random_bytes(40 + diff, 4), std::vector<int>{ 40, 39 + diff }, 16, cases)) return 1;
    }
    printf("%ld cases checked: ok\n", cases);
    return 0;
}
