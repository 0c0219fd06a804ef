// genotype_quality_check.cpp — mtr_amd/csrc/genotype_quality.h on the host, a program of its own (tests/test_genotype_quality_host.py builds it
// with g++, plain and under the address and undefined-behaviour sanitizers).  Three parts:
//   the score      gq_fill - the quality-weighted banded fill in the kernels' schedule - against a full matrix written here, over seeded pairs of
//                  lengths 0..70 with band_extra chosen so that the band is 1, 31 .. 33, 63 .. 65 and 127 .. 129 diagonals wide among others
//                  (the borders of the kernels' buckets; 255 .. 257 need longer sequences and get a few of 0..300), qualities 0..93 and none,
//                  and the two properties of the definition; the same pairs on the 64 lanes of a whole wavefront with one and with two pairs of
//                  diagonals a lane (gq_step_lane: the <1, 1> and <1, 2> shapes' step with its neighbour wiring); and four tasks stepped side by
//                  side as the four rows of a wavefront step - or two as its halves - each holding its values once it is done
//   T              against its formula
//   the locus      gq_add / gq_merge / gq_finish and gq_entry against a naive loop over seeded scores, ties everywhere
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../mtr_amd/csrc/genotype_quality.h"

static long long checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

typedef std::vector<uint8_t> Seq;

// the definition, cell by cell over the whole matrix, infinities outside the band
static long long full_score(const Seq &W, const Seq *Q, const Seq &C, const GqParams &p)
{
    const int n = (int)W.size(), m = (int)C.size();
    const long long INF = 1ll << 40;
    const int dlo = std::min(0, m - n) - p.band_extra, dhi = std::max(0, m - n) + p.band_extra;
    auto w = [&](int k) { return Q ? std::min(std::max((int)(*Q)[(size_t)k], 1), p.qual_cap) : p.qual_cap; };
    auto gamma = [&](int i) { if (n == 0) return 1; if (i == 0) return w(0); if (i == n) return w(n - 1); return std::min(w(i - 1), w(i)); };
    std::vector<std::vector<long long>> D((size_t)n + 1, std::vector<long long>((size_t)m + 1, INF));
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= m; j++) {
            if (j - i < dlo || j - i > dhi) continue;
            if (i == 0 && j == 0) { D[0][0] = 0; continue; }
            long long best = INF;
            if (i >= 1 && j >= 1) best = std::min(best, D[(size_t)i - 1][(size_t)j - 1] + (W[(size_t)i - 1] != C[(size_t)j - 1] ? w(i - 1) : 0));
            if (i >= 1) best = std::min(best, D[(size_t)i - 1][(size_t)j] + std::min(w(i - 1), p.gap_cap));
            if (j >= 1) best = std::min(best, D[(size_t)i][(size_t)j - 1] + std::min(gamma(i), p.gap_cap));
            D[(size_t)i][(size_t)j] = std::min(best, INF);
        }
    return D[(size_t)n][(size_t)m];
}

static Seq random_seq(std::mt19937 &rng, int n, int alphabet)
{
    Seq s((size_t)n);
    for (auto &c : s) c = (uint8_t)(rng() % (unsigned)alphabet);
    return s;
}
static Seq relative(std::mt19937 &rng, const Seq &s, int n, int edits)
{
    Seq w = s;
    for (int k = 0; k < edits && !w.empty(); k++) {
        const size_t at = rng() % w.size();
        switch (rng() % 3) { case 0: w[at] = (uint8_t)(rng() % 4); break; case 1: w.erase(w.begin() + (long)at); break; default: w.insert(w.begin() + (long)at, (uint8_t)(rng() % 4)); }
    }
    while ((int)w.size() > n) w.pop_back();
    while ((int)w.size() < n) w.push_back((uint8_t)(rng() % 4));
    return w;
}
static Seq random_quals(std::mt19937 &rng, int n)
{
    static const uint8_t special[6] = { 0, 1, 2, 40, 41, 93 };
    Seq q((size_t)n);
    const int kind = (int)(rng() % 3);
    for (auto &v : q) v = kind == 0 ? (uint8_t)(rng() % 94) : kind == 1 ? special[rng() % 6] : (uint8_t)(2 + rng() % 10);
    return q;
}

static int32_t by_fill(const Seq &W, const Seq *Q, const Seq &C, const GqParams &p)
{
    const int n = (int)W.size(), m = (int)C.size();
    int32_t E[128], O[128];
    CHECK(!ba_skipped(n, m, p.band_extra), "n %d m %d extra %d", n, m, p.band_extra);
    return gq_fill(n, m, W.data(), Q ? Q->data() : nullptr, C.data(), p, E, O);
}

// one task on the 64 lanes of a whole wavefront, CPL pairs of diagonals a lane, as the <1, CPL> shapes run it: gq_step_lane with the one value that
// comes from the lane beside (the kernel's wavefront shift), BA_INF at the wavefront's ends
template <int CPL>
static int32_t by_lanes(const Seq &W, const Seq *Q, const Seq &C, const GqParams &p)
{
    const int n = (int)W.size(), m = (int)C.size();
    const BaBand band = ba_band(n, m, p.band_extra);
    CHECK(ba_width(band) <= 128 * CPL, "n %d m %d extra %d", n, m, p.band_extra);
    int32_t E[64][CPL], O[64][CPL];
    for (int l = 0; l < 64; l++) for (int k = 0; k < CPL; k++) E[l][k] = O[l][k] = BA_INF;
    for (int32_t s = 0; s <= n + m; s++) {
        int32_t neighbour[64];
        const bool even = ((s - band.dlo) & 1) == 0;
        for (int l = 0; l < 64; l++) neighbour[l] = even ? (l > 0 ? O[l - 1][CPL - 1] : BA_INF) : (l < 63 ? E[l + 1][0] : BA_INF);
        for (int l = 0; l < 64; l++) gq_step_lane<CPL>(s, l, n, m, band, E[l], O[l], neighbour[l], W.data(), Q ? Q->data() : nullptr, C.data(), p);
    }
    const int32_t e = gq_end_diagonal(n, m, band), pair = e >> 1;
    return (e & 1) ? O[pair / CPL][pair % CPL] : E[pair / CPL][pair % CPL];
}

static void check_pair(std::mt19937 &rng, int n, int m, int extra, int round)
{
    const Seq W = random_seq(rng, n, round % 5 == 0 ? 2 : 4);
    const Seq C = round % 3 == 0 ? random_seq(rng, m, 4) : relative(rng, W, m, (int)(rng() % 12));
    const Seq Q = random_quals(rng, n);
    const int qual_cap = 1 + (int)(rng() % 93), gap_cap = 1 + (int)(rng() % (unsigned)qual_cap);
    const GqParams p = { extra, round % 7 == 0 ? 40 : qual_cap, round % 7 == 0 ? 20 : gap_cap, 60 };
    const bool with_q = round % 4 != 3;
    const long long want = full_score(W, with_q ? &Q : nullptr, C, p);
    const int32_t got = by_fill(W, with_q ? &Q : nullptr, C, p);
    CHECK(got == want, "n %d m %d extra %d caps %d %d: %d, the definition gives %lld", n, m, extra, p.qual_cap, p.gap_cap, got, want);
    const Seq *q = with_q ? &Q : nullptr;
    if (ba_width(ba_band(n, m, extra)) <= 128) CHECK(by_lanes<1>(W, q, C, p) == want, "n %d m %d extra %d: one pair a lane gives %d, the definition %lld", n, m, extra, by_lanes<1>(W, q, C, p), want);
    CHECK(by_lanes<2>(W, q, C, p) == want, "n %d m %d extra %d: two pairs a lane give %d, the definition %lld", n, m, extra, by_lanes<2>(W, q, C, p), want);
    // the properties: all weights 1 is the unit-cost banded distance (ba_fill's), one constant quality c <= gap_cap is c times that
    const GqParams one = { extra, 1, 1, 60 };
    std::vector<int32_t> E(256), O(256); std::vector<uint32_t> dirs((size_t)ba_dir_words(n, m, 2));
    const int32_t unit = ba_fill(n, m, W.data(), C.data(), ba_band(n, m, extra), 2, E.data(), O.data(), dirs.data());
    CHECK(by_fill(W, &Q, C, one) == unit, "n %d m %d extra %d: weights 1 give %d, the unit distance is %d", n, m, extra, by_fill(W, &Q, C, one), unit);
    if (n > 0) {
        const int c = 1 + (int)(rng() % (unsigned)p.gap_cap);
        const Seq flat((size_t)n, (uint8_t)c);
        CHECK(by_fill(W, &flat, C, p) == c * unit, "n %d m %d extra %d: constant %d", n, m, extra, c);
    }
    checked++;
}

// ROWS tasks as the rows or halves of a wavefront, L = 64 / ROWS lanes each: every one steps to the longest task's last anti-diagonal, one past
// its own keeps what it has
template <int ROWS>
static void check_rows(const Seq (&W)[4], const Seq (&Q)[4], const Seq (&C)[4], const GqParams &p)
{
    constexpr int L = 64 / ROWS;
    int32_t E[ROWS][L], O[ROWS][L], n[ROWS], m[ROWS], last = 0;
    BaBand band[ROWS];
    for (int g = 0; g < ROWS; g++) {
        n[g] = (int)W[g].size(); m[g] = (int)C[g].size(); band[g] = ba_band(n[g], m[g], p.band_extra);
        CHECK(ba_width(band[g]) <= 2 * L, "extra %d", p.band_extra);
        last = std::max(last, n[g] + m[g]);
        for (int r = 0; r < L; r++) E[g][r] = O[g][r] = BA_INF;
    }
    for (int32_t s = 0; s <= last; s++)
        for (int g = 0; g < ROWS; g++) {
            int32_t below[L], above[L];
            for (int r = 0; r < L; r++) { below[r] = r > 0 ? O[g][r - 1] : BA_INF; above[r] = r < L - 1 ? E[g][r + 1] : BA_INF; }
            for (int r = 0; r < L; r++) {
                int32_t e2 = E[g][r], o2 = O[g][r];
                gq_step(s, r, n[g], m[g], band[g], e2, o2, below[r], above[r], W[g].data(), Q[g].data(), C[g].data(), p);
                if (s <= n[g] + m[g]) { E[g][r] = e2; O[g][r] = o2; }
            }
        }
    for (int g = 0; g < ROWS; g++) {
        const int32_t e = gq_end_diagonal(n[g], m[g], band[g]);
        const long long got = (e & 1) ? O[g][e >> 1] : E[g][e >> 1], want = full_score(W[g], &Q[g], C[g], p);
        CHECK(got == want, "row %d: n %d m %d extra %d: %lld, the definition gives %lld", g, n[g], m[g], p.band_extra, got, want);
        checked++;
    }
}

static void check_scores()
{
    std::mt19937 rng(20250117u);
    static const int widths[14] = { 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 9, 17, 45 };
    for (int round = 0; round < 10500; round++) {
        const int n = (int)(rng() % 71), m = (int)(rng() % 71), diff = std::abs(n - m);
        int extra = (int)(rng() % 65);
        const int width = widths[round % 14];                                   // the band |m - n| + 2 * extra + 1 at a bucket's border, where the lengths allow it
        if (round % 2 == 0 && width > diff && (width - diff - 1) % 2 == 0 && (width - diff - 1) / 2 <= BA_MAX_EXTRA) extra = (width - diff - 1) / 2;
        check_pair(rng, n, m, extra, round);
    }
    for (int round = 0; round < 60; round++) {                                  // 255 .. 257 diagonals: 256 is the last band that is scored
        const int diff = 200 + (int)(rng() % 54), n = (int)(rng() % 40), extra = (256 - diff - 1) / 2 - (int)(round % 4 == 3);       // (extra >= 1 before the step down)
        if (round % 2) check_pair(rng, n, n + diff, extra, round); else check_pair(rng, n + diff, n, extra, round);
        CHECK(ba_skipped(n, n + 256, 0) && !ba_skipped(n, n + 255, 0), "the skip rule");
    }
    for (int round = 0; round < 400; round++) {
        const bool halves = round % 4 >= 2;                                     // two tasks in halves of 32 lanes: bands of up to 64 diagonals
        const int extra = halves ? 16 + (int)(rng() % 12) : (int)(rng() % 12);
        Seq W[4], Q[4], C[4];
        for (int g = 0; g < 4; g++) {
            const int n = (int)(rng() % (g == (halves ? (round >> 2) % 2 : round % 4) ? 70u : 12u));        // one long task beside short ones, empty ones among them
            const int m = std::max(0, n + (int)(rng() % 9) - 4);
            W[g] = random_seq(rng, n, 4); C[g] = rng() % 4 ? relative(rng, W[g], m, (int)(rng() % 8)) : random_seq(rng, m, 4); Q[g] = random_quals(rng, n);
        }
        const GqParams p = { extra, 40, 20, 60 };
        if (halves) check_rows<2>(W, Q, C, p); else check_rows<4>(W, Q, C, p);
    }
}

static void check_T()
{
    for (int d = 0; d < 40; d++) {
        const int want = d >= 10 ? 0 : (int)std::lround(10.0 * std::log10(1.0 + std::pow(10.0, -d / 10.0)));
        CHECK(gq_T(d) == want, "T[%d] = %d, the formula gives %d", d, gq_T(d), want);
        checked++;
    }
}

static void check_loci()
{
    std::mt19937 rng(99u);
    static const int T[10] = { 3, 3, 2, 2, 1, 1, 1, 1, 1, 1 };
    for (int round = 0; round < 3000; round++) {
        const int z = round % 5 == 0 ? 0 : round % 5 == 1 ? 1 : 2, S = (int)(rng() % (round % 9 ? 12u : 200u)), read_cap = 1 + (int)(rng() % (round % 2 ? 12u : 200u));
        const int spread = 1 + (int)(rng() % (round % 3 ? 14u : 3000u));
        std::vector<int32_t> s0((size_t)S), s1((size_t)S); std::vector<int> al((size_t)S);
        for (int e = 0; e < S; e++) {
            const bool scored = z > 0 && rng() % 5 != 0;
            s0[(size_t)e] = scored ? (int32_t)(rng() % (unsigned)spread) : -1;
            s1[(size_t)e] = scored && z == 2 ? (rng() % 3 ? (int32_t)(rng() % (unsigned)spread) : s0[(size_t)e]) : -1;
            al[(size_t)e] = (int)(rng() % 2);
        }
        // the kernel's way: 64 lanes of partial sums, merged
        GqSums lanes[64] = {}, t = { 0, 0, 0, 0, 0 };
        for (int e = 0; e < S; e++) gq_add(lanes[e % 64], z, s0[(size_t)e], s1[(size_t)e], read_cap);
        for (int k = 0; k < 64; k++) gq_merge(t, lanes[k]);
        int64_t raw[3], pl[3], gq; uint8_t gt;
        gq_finish(z, t, raw, pl, gt, gq);
        // the definition, naively
        long long w[3] = { 0, 0, 0 }; int n_scored = 0, n_un = 0;
        for (int e = 0; e < S; e++) {
            uint8_t best; int32_t margin;
            gq_entry(z, s0[(size_t)e], s1[(size_t)e], al[(size_t)e], best, margin);
            const bool scored = s0[(size_t)e] >= 0;
            int wb = al[(size_t)e], wm = 0;
            if (scored && z == 1) wb = 0;
            if (scored && z == 2) { wm = std::abs(s0[(size_t)e] - s1[(size_t)e]); if (s0[(size_t)e] < s1[(size_t)e]) wb = 0; else if (s1[(size_t)e] < s0[(size_t)e]) wb = 1; }
            CHECK(best == wb && margin == wm, "round %d entry %d: best %d/%d margin %d/%d", round, e, best, wb, margin, wm);
            if (z == 0) continue;
            if (!scored) { n_un++; continue; }
            n_scored++;
            const int x0 = std::min(s0[(size_t)e], read_cap), x1 = std::min(s1[(size_t)e], read_cap);
            w[0] += x0;
            if (z == 2) { const int d = std::abs(x0 - x1); w[1] += std::min(x0, x1) + 3 - (d < 10 ? T[d] : 0); w[2] += x1; }
        }
        CHECK(t.scored == n_scored && t.unscored == n_un, "round %d: counts", round);
        if (z == 2) {
            static const int order[3] = { 1, 0, 2 };
            int g = 1;
            for (int k : order) if (w[k] < w[g]) g = k;
            long long least = -1;
            for (int k = 0; k < 3; k++) { CHECK(raw[k] == w[k] && pl[k] == w[k] - w[g], "round %d: raw / pl %d", round, k); if (k != g && (least < 0 || pl[k] < least)) least = pl[k]; }
            CHECK(gt == g && gq == least, "round %d: gt %d/%d gq %lld/%lld", round, gt, g, (long long)gq, least);
        } else if (z == 1) CHECK(raw[0] == w[0] && raw[1] == -1 && raw[2] == -1 && pl[0] == 0 && pl[1] == -1 && pl[2] == -1 && gt == 0 && gq == -1, "round %d: zygosity 1", round);
        else CHECK(raw[0] == -1 && raw[1] == -1 && raw[2] == -1 && pl[0] == -1 && pl[1] == -1 && pl[2] == -1 && gt == 255 && gq == -1 && t.scored == 0 && t.unscored == 0, "round %d: zygosity 0", round);
        checked++;
    }
}

int main()
{
    check_scores();
    check_T();
    check_loci();
    printf("%lld cases checked: ok\n", checked);
    return 0;
}
