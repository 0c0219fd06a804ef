// seq_calls_check.cpp — mtr_amd/csrc/seq_calls.h on the host, a program of its own (tests/test_seq_calls_host.py builds it with g++, plain and
// under the address and undefined-behaviour sanitizers).  Three parts:
//   the distance   sq_fill - the banded, clamped fill in the kernels' schedule, rows of a wavefront and whole wavefronts alike - against a full
//                  matrix written here, over seeded pairs of lengths 0..70, K in {0, 1, 5, 31, 32, 254}, length differences of either sign,
//                  |difference| = K and K + 1 among them; and four tasks stepped side by side as the four rows of a wavefront step - or two as
//                  its halves - each holding its values once it is done
//   the pair index sq_pair_index against counting, sq_pair_at as its inverse, for every S up to SQ_MAX_MEMBERS
//   the split      sq_split and sq_place against a naive triple loop over seeded matrices, ties everywhere
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../mtr_amd/csrc/seq_calls.h"

static long long checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static int full_lev(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b)
{
    const size_t n = a.size(), m = b.size();
    std::vector<std::vector<int>> D(n + 1, std::vector<int>(m + 1, 0));
    for (size_t i = 0; i <= n; i++)
        for (size_t j = 0; j <= m; j++)
            D[i][j] = i == 0 || j == 0 ? (int)(i + j) : std::min({ D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1 });
    return D[n][m];
}

static int definition(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, int K)
{
    const long long diff = std::llabs((long long)a.size() - (long long)b.size());
    if (diff > K) return K + 1;
    return std::min(full_lev(a, b), K + 1);
}

static std::vector<uint8_t> random_seq(std::mt19937 &rng, int n, int alphabet)
{
    std::vector<uint8_t> s((size_t)n);
    for (auto &c : s) c = (uint8_t)(rng() % (unsigned)alphabet);
    return s;
}
// a relative of s with about `edits` edits, brought to exactly n bases
static std::vector<uint8_t> relative(std::mt19937 &rng, const std::vector<uint8_t> &s, int n, int edits)
{
    std::vector<uint8_t> w = s;
    for (int k = 0; k < edits && !w.empty(); k++) {
        const size_t at = rng() % w.size();
        switch (rng() % 3) { case 0: w[at] = (uint8_t)(rng() % 4); break; case 1: w.erase(w.begin() + (long)at); break; default: w.insert(w.begin() + (long)at, (uint8_t)(rng() % 4)); }
    }
    while ((int)w.size() > n) w.pop_back();
    while ((int)w.size() < n) w.push_back((uint8_t)(rng() % 4));
    return w;
}

static int by_fill(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, int K)
{
    const int n = (int)a.size(), m = (int)b.size();
    if (sq_far(n, m, K)) return K + 1;
    if (n == 0 || m == 0) return n + m;                                       // (resolved at once by the task kernel)
    int32_t E[128], O[128];
    CHECK(ba_width(sq_band(n, m, K)) <= K + 1 && (ba_width(sq_band(n, m, K)) + 1) / 2 <= 128, "n %d m %d K %d", n, m, K);
    return sq_fill(n, m, a.data(), b.data(), K, E, O);
}

// ROWS tasks (four or two of the four given) as the rows or halves of a wavefront, L = 64 / ROWS lanes each: every one steps to the longest
// task's last anti-diagonal, one past its own keeps what it has
template <int ROWS>
static void check_rows(const std::vector<uint8_t> (&a)[4], const std::vector<uint8_t> (&b)[4], int K)
{
    constexpr int L = 64 / ROWS;
    int32_t E[ROWS][L], O[ROWS][L], n[ROWS], m[ROWS], last = 0;
    BaBand band[ROWS];
    for (int g = 0; g < ROWS; g++) {
        n[g] = (int)a[g].size(); m[g] = (int)b[g].size(); band[g] = sq_band(n[g], m[g], K);
        CHECK(ba_width(band[g]) <= 2 * L, "K %d", K);
        last = std::max(last, n[g] + m[g]);
        for (int r = 0; r < L; r++) E[g][r] = O[g][r] = BA_INF;
    }
    for (int32_t s = 0; s <= last; s++)
        for (int g = 0; g < ROWS; g++) {
            int32_t below[L], above[L];
            for (int r = 0; r < L; r++) { below[r] = r > 0 ? O[g][r - 1] : BA_INF; above[r] = r < L - 1 ? E[g][r + 1] : BA_INF; }
            for (int r = 0; r < L; r++) {
                int32_t e2 = E[g][r], o2 = O[g][r];
                sq_step(s, r, n[g], m[g], band[g], e2, o2, below[r], above[r], a[g].data(), b[g].data());
                if (s <= n[g] + m[g]) { E[g][r] = e2; O[g][r] = o2; }
            }
        }
    for (int g = 0; g < ROWS; g++) {
        const int32_t e = sq_end_diagonal(n[g], m[g], band[g]);
        const int got = sq_clamp((e & 1) ? O[g][e >> 1] : E[g][e >> 1], K), want = definition(a[g], b[g], K);
        CHECK(got == want, "row %d: n %d m %d K %d: %d, the definition gives %d", g, n[g], m[g], K, got, want);
        checked++;
    }
}

static void check_distances()
{
    std::mt19937 rng(20240521u);
    static const int Ks[6] = { 0, 1, 5, 31, 32, 254 };
    for (int round = 0; round < 1900; round++)
        for (int K : Ks) {
            const int n = (int)(rng() % 71);
            int m;
            switch (round % 6) {                                                // either sign; |difference| = K and K + 1; anything
                case 0: m = n + K; break;
                case 1: m = n - K; break;
                case 2: m = n + K + 1; break;
                case 3: m = n - K - 1; break;
                case 4: m = n + (int)(rng() % 7) - 3; break;
                default: m = (int)(rng() % 71); break;
            }
            if (m < 0 || m > 70) m = (int)(rng() % 71);
            const std::vector<uint8_t> a = random_seq(rng, n, round % 5 == 0 ? 2 : 4);
            const std::vector<uint8_t> b = round % 3 == 0 ? random_seq(rng, m, 4) : relative(rng, a, m, (int)(rng() % (unsigned)(K + 3)));
            const int got = by_fill(a, b, K), want = definition(a, b, K);
            CHECK(got == want, "n %d m %d K %d: %d, the definition gives %d", n, m, K, got, want);
            CHECK(by_fill(b, a, K) == want, "n %d m %d K %d: not symmetric", n, m, K);
            checked++;
        }
    for (int round = 0; round < 400; round++) {
        const bool halves = round % 4 >= 2;                                     // two tasks in halves of 32 lanes: bands of up to 64 diagonals
        const int K = halves ? (round % 8 >= 6 ? 63 : 32 + (int)(rng() % 31)) : round % 2 ? 31 : 5 + (int)(rng() % 20);
        std::vector<uint8_t> a[4], b[4];
        for (int g = 0; g < 4; g++) {
            const int n = 1 + (int)(rng() % (g == (halves ? (round >> 2) % 2 : round % 4) ? 70u : 12u));    // one long task beside short ones
            const int m = std::max(1, n + (int)(rng() % 9) - 4);
            a[g] = random_seq(rng, n, 4); b[g] = rng() % 4 ? relative(rng, a[g], m, (int)(rng() % 8)) : random_seq(rng, m, 4);
            if (std::abs(n - m) > K) b[g] = relative(rng, a[g], n, 2);
        }
        if (halves) check_rows<2>(a, b, K); else check_rows<4>(a, b, K);
    }
}

static void check_pair_index()
{
    for (int S = 2; S <= SQ_MAX_MEMBERS; S++) {
        int64_t q = 0;
        for (int t = 0; t < S; t++)
            for (int u = t + 1; u < S; u++, q++) {
                CHECK(sq_pair_index(S, t, u) == q, "S %d t %d u %d", S, t, u);
                int32_t t2, u2;
                sq_pair_at(S, q, t2, u2);
                CHECK(t2 == t && u2 == u, "S %d q %lld: (%d, %d), not (%d, %d)", S, (long long)q, t2, u2, t, u);
            }
        CHECK(q == sq_pairs(S), "S %d", S);
        checked++;
    }
}

static void check_split()
{
    std::mt19937 rng(77u);
    const int stride = SQ_MAX_MEMBERS;
    std::vector<uint8_t> mat((size_t)stride * stride);
    for (int round = 0; round < 600; round++) {
        const int S = round < 8 ? (round < 4 ? round : SQ_MAX_MEMBERS - (round - 4)) : (int)(rng() % 20);
        const int spread = 1 + (int)(rng() % (round % 3 ? 4u : 255u));          // a small range of values: ties
        const int groups = 1 + (int)(rng() % 3);
        std::fill(mat.begin(), mat.end(), (uint8_t)0xee);
        for (int t = 0; t < S; t++)
            for (int u = t; u < S; u++) {
                const int far = (t % groups != u % groups) ? (int)(rng() % 3) * spread : 0;
                const uint8_t v = t == u ? 0 : (uint8_t)std::min(255, far + (int)(rng() % (unsigned)spread));
                mat[(size_t)t * stride + u] = mat[(size_t)u * stride + t] = v;
            }
        const SqParams p = { 254, 1 + (int)(rng() % 4), (int)(rng() % 51), 1 + (int)(rng() % 3), (int)(rng() % 101) };
        const SqSplit r = sq_split(mat.data(), stride, S, p);
        // the definition, naively
        SqSplit w = { 0, -1, -1, 0, 0, 0, 0 };
        if (S >= p.min_support) {
            long long best1 = -1;
            for (int c = 0; c < S; c++) {
                long long cost = 0;
                for (int u = 0; u < S; u++) cost += mat[(size_t)c * stride + u];
                if (best1 < 0 || cost < best1) { best1 = cost; w.c0 = c; }
            }
            w.zygosity = 1; w.cost1 = w.cost2 = best1; w.n0 = S;
            long long best2 = -1;
            for (int c0 = 0; c0 < S; c0++)
                for (int c1 = c0 + 1; c1 < S; c1++) {
                    long long cost2 = 0, n0 = 0;
                    for (int u = 0; u < S; u++) {
                        const int x = mat[(size_t)c0 * stride + u], y = mat[(size_t)c1 * stride + u];
                        if (x <= y) { n0++; cost2 += x; } else cost2 += y;
                    }
                    const long long least = std::min<long long>(n0, S - n0);
                    if (least < p.min_support || least * 100 < (long long)p.min_percent * S || mat[(size_t)c0 * stride + c1] < p.min_sep || cost2 * 100 > best1 * (100 - p.min_gain)) continue;
                    if (best2 < 0 || cost2 < best2) { best2 = cost2; w.zygosity = 2; w.c0 = c0; w.c1 = c1; w.n0 = (int32_t)n0; w.n1 = S - (int32_t)n0; w.cost2 = cost2; }
                }
        }
        CHECK(r.zygosity == w.zygosity && r.c0 == w.c0 && r.c1 == w.c1 && r.n0 == w.n0 && r.n1 == w.n1 && r.cost1 == w.cost1 && r.cost2 == w.cost2,
              "round %d S %d: zygosity %d/%d medoids (%d, %d)/(%d, %d) sizes (%d, %d)/(%d, %d) costs (%lld, %lld)/(%lld, %lld)", round, S, r.zygosity, w.zygosity, r.c0, r.c1, w.c0,
              w.c1, r.n0, r.n1, w.n0, w.n1, (long long)r.cost1, (long long)r.cost2, (long long)w.cost1, (long long)w.cost2);
        // the partition: a permutation, allele 0 in front, list order within either allele
        std::vector<int> at((size_t)S, -1);
        int before0 = 0;
        for (int u = 0; u < S; u++) {
            const bool first = r.zygosity < 2 || sq_in_first(mat.data(), stride, r.c0, r.c1, u);
            const int32_t pos = sq_place(r, u, first, before0);
            CHECK(pos >= 0 && pos < S && at[(size_t)pos] < 0, "round %d: member %d placed at %d", round, u, pos);
            at[(size_t)pos] = u;
            if (r.zygosity == 2) CHECK(first == (pos < r.n0), "round %d: member %d of allele %d at %d, n0 %d", round, u, first ? 0 : 1, pos, r.n0);
            before0 += first ? 1 : 0;
        }
        for (int k = 1; k < S; k++) CHECK(r.zygosity < 2 ? at[(size_t)k] == k : (k == r.n0 || at[(size_t)k - 1] < at[(size_t)k]), "round %d: place %d out of list order", round, k);
        checked++;
    }
}

int main()
{
    check_distances();
    check_pair_index();
    check_split();
    printf("%lld cases checked: ok\n", checked);
    return 0;
}
