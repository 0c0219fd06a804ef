// allele_split_check.cpp — the split of one locus' sorted values (mtr_amd/csrc/allele_split.h) for the host: a program of its own (the form a
// sanitizer build runs) that holds allele_seg, allele_admissible, allele_better and allele_best_split - the functions mtr_k_allele_split runs,
// one share of the splits per lane - to brute force written here from the definition of include/mtr_hip.h: medians by index, sad by explicit
// sums, every split in turn.  Seeded lists of 0 .. 70 values: values in 0 .. 5 (runs of equal values, ties of the cost), two noisy clusters,
// uniform in 0 .. 833 333; every combination of min_support 1 / 3, min_percent 0 / 20 / 50 and min_sep 1 / 5.  The prefix array holds exactly
// S + 1 entries and the values exactly S, so a function that reads beyond them trips the address sanitizer.  The best split is also put together
// from 1, 7, 64 and 256 strided shares, as the kernel's lanes do.
#include "../mtr_amd/csrc/allele_split.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint32_t g_rng = 20260u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }      // lo .. hi

static long g_cases = 0, g_two = 0, g_one = 0, g_ties = 0, g_refused[4] = { 0, 0, 0, 0 };

static int64_t brute_med(const std::vector<int32_t> &v, int64_t i, int64_t j) { return v[(size_t)(i + (j - i - 1) / 2)]; }
static int64_t brute_sad(const std::vector<int32_t> &v, int64_t i, int64_t j)
{
    const int64_t m = brute_med(v, i, j);
    int64_t s = 0;
    for (int64_t t = i; t < j; t++) s += std::llabs((long long)v[(size_t)t] - (long long)m);
    return s;
}

static bool one(const std::vector<int32_t> &v, const AlleleRule &r, const char *what)
{
    const int64_t S = (int64_t)v.size();
    std::vector<int64_t> pre((size_t)S + 1, 0);
    for (int64_t t = 0; t < S; t++) pre[(size_t)t + 1] = pre[(size_t)t] + v[(size_t)t];
    // brute force
    int64_t bk = 0, bcost = 0; bool tie = false;
    for (int64_t k = 1; k < S; k++) {
        const int64_t small = std::min(k, S - k);
        const bool c[4] = { v[(size_t)k - 1] < v[(size_t)k], small >= r.min_support, small * 100 >= (int64_t)r.min_percent * S,
                            brute_med(v, k, S) - brute_med(v, 0, k) >= r.min_sep };
        const int failed = !c[0] + !c[1] + !c[2] + !c[3];
        if (failed == 1) for (int q = 0; q < 4; q++) if (!c[q]) g_refused[q]++;
        AlleleSplit s = allele_no_split();
        const bool adm = allele_admissible(v.data(), pre.data(), S, k, r, s);
        if (adm != (failed == 0)) { printf("%s: S %ld k %ld: admissible %d, brute force %d\n", what, (long)S, (long)k, (int)adm, (int)(failed == 0)); return false; }
        if (failed) continue;
        const int64_t cost = brute_sad(v, 0, k) + brute_sad(v, k, S);
        if (s.cost != cost || s.k != k || s.med[0] != brute_med(v, 0, k) || s.med[1] != brute_med(v, k, S)) {
            printf("%s: S %ld k %ld: cost %ld against %ld\n", what, (long)S, (long)k, (long)s.cost, (long)cost); return false;
        }
        if (bk == 0 || cost < bcost) { bk = k; bcost = cost; tie = false; }
        else if (cost == bcost) tie = true;
    }
    if (S > 0) {
        const AlleleSeg all = allele_seg(v.data(), pre.data(), 0, S);
        if (all.sad != brute_sad(v, 0, S) || all.med != brute_med(v, 0, S)) { printf("%s: S %ld: cost1 %ld against %ld\n", what, (long)S, (long)all.sad, (long)brute_sad(v, 0, S)); return false; }
    }
    static const int64_t shares[4] = { 1, 7, 64, 256 };
    for (int64_t step : shares) {
        AlleleSplit best = allele_no_split();
        for (int64_t first = step; first >= 1; first--) {                 // (the shares in descending order: the tie rule must not lean on the order)
            const AlleleSplit s = allele_best_split(v.data(), pre.data(), S, r, first, step);
            if (allele_better(s.cost, s.k, best.cost, best.k)) best = s;
        }
        if (best.k != bk || (bk > 0 && best.cost != bcost)) { printf("%s: S %ld, %ld shares: k %ld cost %ld against k %ld cost %ld\n", what, (long)S, (long)step, (long)best.k, (long)best.cost, (long)bk, (long)bcost); return false; }
    }
    g_cases++; g_two += bk > 0; g_one += bk == 0 && S > 0; g_ties += tie;
    return true;
}

int main()
{
    static const int sup[2] = { 1, 3 }, pct[3] = { 0, 20, 50 }, sep[2] = { 1, 5 };
    for (int rep = 0; rep < 900; rep++) {
        const int S = rep < 71 ? rep : rnd_in(0, 70), kind = rep % 3;
        std::vector<int32_t> v((size_t)S);
        for (int32_t &x : v) x = kind == 0 ? rnd_in(0, 5) : kind == 1 ? (rnd_in(0, 9) < 4 ? 35 : 20) + rnd_in(-2, 2) : rnd_in(0, 833333);
        std::sort(v.begin(), v.end());
        for (int a = 0; a < 2; a++) for (int b = 0; b < 3; b++) for (int c = 0; c < 2; c++) {
            const AlleleRule r = { sup[a], pct[b], sep[c] };
            if (!one(v, r, kind == 0 ? "values 0..5" : kind == 1 ? "two clusters" : "uniform")) return 1;
        }
    }
    // by hand: the definition's examples
    {
        const AlleleRule r = { 3, 20, 2 };
        const std::vector<int32_t> v = { 10, 10, 10, 40, 40, 40, 70, 70, 70 };
        std::vector<int64_t> pre(10, 0);
        for (size_t t = 0; t < 9; t++) pre[t + 1] = pre[t] + v[t];
        const AlleleSplit s = allele_best_split(v.data(), pre.data(), 9, r, 1, 1);
        if (s.k != 3 || s.cost != 90 || s.med[0] != 10 || s.med[1] != 40 || allele_seg(v.data(), pre.data(), 0, 9).sad != 180) { printf("the tie by hand: k %ld cost %ld\n", (long)s.k, (long)s.cost); return 1; }
        // the largest values the call takes: 2^31 - 1 twice against 0 twice stays exact
        const std::vector<int32_t> w = { 0, 0, INT32_MAX, INT32_MAX };
        std::vector<int64_t> pw(5, 0);
        for (size_t t = 0; t < 4; t++) pw[t + 1] = pw[t] + w[t];
        const AlleleRule r1 = { 1, 0, 1 };
        if (allele_seg(w.data(), pw.data(), 0, 4).sad != 2 * (int64_t)INT32_MAX || allele_best_split(w.data(), pw.data(), 4, r1, 1, 1).k != 2) { printf("the largest values\n"); return 1; }
    }
    if (g_two < 500 || g_one < 500 || g_ties < 50 || g_refused[0] < 50 || g_refused[1] < 50 || g_refused[2] < 50 || g_refused[3] < 50) {
        printf("a degenerate run: %ld %ld %ld, refused %ld %ld %ld %ld\n", g_two, g_one, g_ties, g_refused[0], g_refused[1], g_refused[2], g_refused[3]); return 1;
    }
    printf("%ld cases checked (%ld split in two, %ld ties of the least cost; refused alone by value, support, percent, distance: %ld %ld %ld %ld): ok\n",
           g_cases, g_two, g_ties, g_refused[0], g_refused[1], g_refused[2], g_refused[3]);
    return 0;
}
