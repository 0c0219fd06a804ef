// seq_calls.h — the sequence allele calls' arithmetic: the saturated edit distance D(t, u) = min(lev(W_t, W_u), K + 1) between two oriented
// windows, the place of a pair in a locus' upper triangle, the one- and two-medoid selection over a locus' distances and the stable partition.
// Plain C++, nothing of HIP: the same functions compile into the gfx950 kernels (seq_calls.hip.inc) and into a host program
// (tests/seq_calls_check.cpp), which holds them to a full-matrix Levenshtein and to a naive triple loop.
//
// The definition is include/mtr_hip.h's ("sequence allele calls").  The cell, the band's shape and the anti-diagonal schedule - pairs of
// diagonals (E, O), one neighbour value per step - are banded_align.h's, run WITHOUT directions: nothing is kept per cell.
//   distance    D = K + 1 by definition when a window exceeds BA_MAX_WINDOW or |n - m| > K (sq_far).  Else the banded fill over the diagonals
//               ba_band(n, m, (K - |m - n|) >> 1): |m - n| + 2 * extra + 1 <= K + 1 diagonals.  A path of cost c <= K from (0, 0) to (n, m)
//               makes x steps up and y steps left with x + y <= c and |x - y| = |m - n|, so it strays at most (c - |m - n|) / 2 <= extra
//               diagonals beyond the two end diagonals: it never leaves the band, and the banded minimum is lev whenever lev <= K.  When
//               lev > K every banded path costs more than K as well (it is a path of the full matrix), so clamping to K + 1 gives exactly D
//   split       cost(c) = sum over u of D(c, u); for c0 < c1 member u belongs to c0 iff D(c0, u) <= D(c1, u).  The keys below order the
//               candidates exactly as the definition words it: least cost, then the smallest index (indices)
#pragma once
#include "banded_align.h"

#define SQ_MAX_DIST 254            // MTR_SEQ_MAX_DIST: K + 1 fits a byte
#define SQ_MAX_MEMBERS 128         // MTR_SEQ_MAX_MEMBERS: the locus' matrix is at most 16 KiB of bytes
#define SQ_ROW_BAND 32             // the widest band one 16-lane row holds: 16 pairs of diagonals
#define SQ_HALF_BAND 64            // the widest band half a wavefront holds: 32 pairs
#define SQ_BUCKETS 4               // bands of up to SQ_ROW_BAND, SQ_HALF_BAND, 128 (one pair per lane), 256 (two pairs per lane) diagonals
#define SQ_NO_KEY 0xffffffffu

struct SqParams { int32_t max_dist, min_support, min_percent, min_sep, min_gain; };

// ---- the distance -------------------------------------------------------------------------------------------------------------------------
BA_HD int64_t sq_absdiff(int64_t n, int64_t m) { return m > n ? m - n : n - m; }
// is D(t, u) = K + 1 by definition, whatever the windows hold?
BA_HD bool sq_far(int64_t n, int64_t m, int32_t K) { return n > BA_MAX_WINDOW || m > BA_MAX_WINDOW || sq_absdiff(n, m) > K; }
BA_HD BaBand sq_band(int32_t n, int32_t m, int32_t K) { return ba_band(n, m, (K - (int32_t)sq_absdiff(n, m)) >> 1); }
BA_HD int32_t sq_clamp(int32_t d, int32_t K) { return d > K ? K + 1 : d; }
BA_HD int sq_bucket(int32_t width) { return width <= SQ_ROW_BAND ? 0 : width <= SQ_HALF_BAND ? 1 : width <= 128 ? 2 : 3; }

// One step of pair p on anti-diagonal s, whichever parity the task's band gives it: the pair's running values (E, O), `below` = O of pair
// p - 1, `above` = E of pair p + 1 (BA_INF at the band's ends).  Four tasks in the four rows of a wavefront, or two in its halves, step side by
// side through this although their parities differ; a task whose parity is the wavefront's takes the branch of banded_align.h's schedule directly.
BA_HD void sq_step(int32_t s, int32_t p, int32_t n, int32_t m, const BaBand &b, int32_t &E, int32_t &O, int32_t below, int32_t above, const uint8_t *W,
                   const uint8_t *B)
{
    const int par = (s - b.dlo) & 1;
    int dir;
    const int32_t v = ba_step_cell(s, 2 * p + par, n, m, b, par ? O : E, par ? above : O, par ? E : below, W, B, dir);
    if (par) O = v; else E = v;
}
// which pair, and which of its two values, holds D(n, m) after step n + m
BA_HD int32_t sq_end_diagonal(int32_t n, int32_t m, const BaBand &b) { return m - n - b.dlo; }

// the whole fill in the kernels' schedule by ONE thread, for windows that are not sq_far: E, O hold (ba_width + 1) / 2 values each (at most 128).
// Returns D(t, u), clamped.  The kernels run the same steps with pair p in lane p (a row of 16, or the wavefront's 64) or in lane p / 2.
BA_HD int32_t sq_fill(int32_t n, int32_t m, const uint8_t *W, const uint8_t *B, int32_t K, int32_t *E, int32_t *O)
{
    const BaBand b = sq_band(n, m, K);
    const int32_t pairs = (ba_width(b) + 1) >> 1;
    for (int32_t p = 0; p < pairs; p++) E[p] = O[p] = BA_INF;
    for (int32_t s = 0; s <= n + m; s++)
        for (int32_t p = 0; p < pairs; p++)                                     // (a step writes one of E, O and reads the neighbours' other one: any order of p)
            sq_step(s, p, n, m, b, E[p], O[p], p > 0 ? O[p - 1] : BA_INF, p + 1 < pairs ? E[p + 1] : BA_INF, W, B);
    const int32_t e = sq_end_diagonal(n, m, b);
    return sq_clamp((e & 1) ? O[e >> 1] : E[e >> 1], K);
}

// ---- the upper triangle -------------------------------------------------------------------------------------------------------------------
BA_HD int64_t sq_pairs(int64_t S) { return S * (S - 1) / 2; }
BA_HD int64_t sq_row_start(int32_t S, int32_t t) { return (int64_t)t * S - (int64_t)t * (t + 1) / 2; }
BA_HD int64_t sq_pair_index(int32_t S, int32_t t, int32_t u) { return sq_row_start(S, t) + (u - t - 1); }       // t < u
// the pair at place q, 0 <= q < sq_pairs(S): the last row that starts at or before q (rows 0 .. S - 2 hold at least one pair each)
BA_HD void sq_pair_at(int32_t S, int64_t q, int32_t &t, int32_t &u)
{
    int32_t lo = 0, hi = S - 2;
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (sq_row_start(S, mid) <= q) lo = mid; else hi = mid - 1; }
    t = lo; u = lo + 1 + (int32_t)(q - sq_row_start(S, lo));
}

// ---- the medoids ----------------------------------------------------------------------------------------------------------------------------
// Mat: the locus' full symmetric matrix as bytes, D(c, u) = mat[u * stride + c] (the kernel's lanes hold consecutive c: consecutive bytes).
template <class Mat>
BA_HD int32_t sq_cost(Mat mat, int32_t stride, int32_t S, int32_t c)
{
    int32_t sum = 0;
    for (int32_t u = 0; u < S; u++) sum += mat[u * stride + c];
    return sum;
}
// the smallest key is the smallest c of least cost: cost <= 128 * 255 < 2^15
BA_HD uint32_t sq_cost_key(int32_t cost, int32_t c) { return ((uint32_t)cost << 8) | (uint32_t)c; }

template <class Mat>
BA_HD bool sq_in_first(Mat mat, int32_t stride, int32_t c0, int32_t c1, int32_t u) { return mat[u * stride + c0] <= mat[u * stride + c1]; }

template <class Mat>
BA_HD void sq_pair_eval(Mat mat, int32_t stride, int32_t S, int32_t c0, int32_t c1, int32_t &n0, int32_t &cost2)
{
    n0 = 0; cost2 = 0;
    for (int32_t u = 0; u < S; u++) {
        const int32_t a = mat[u * stride + c0], b = mat[u * stride + c1];
        if (a <= b) { n0++; cost2 += a; } else cost2 += b;
    }
}
BA_HD bool sq_admissible(const SqParams &p, int32_t S, int32_t n0, int32_t sep, int64_t cost1, int64_t cost2)
{
    const int64_t least = n0 < S - n0 ? n0 : S - n0;
    return least >= p.min_support && least * 100 >= (int64_t)p.min_percent * S && sep >= p.min_sep && cost2 * 100 <= cost1 * (100 - p.min_gain);
}
// the smallest key is the pair of least cost2, then the smallest c0, then the smallest c1: cost2 < 2^15, c0 and c1 < 2^7
BA_HD uint32_t sq_pair_key(int32_t cost2, int32_t c0, int32_t c1) { return ((uint32_t)cost2 << 14) | ((uint32_t)c0 << 7) | (uint32_t)c1; }

struct SqSplit { int32_t zygosity, c0, c1, n0, n1; int64_t cost1, cost2; };

// the outcome of one locus of S <= SQ_MAX_MEMBERS members by ONE thread; the kernel spreads the candidates over its lanes and reduces the keys
template <class Mat>
BA_HD SqSplit sq_split(Mat mat, int32_t stride, int32_t S, const SqParams &p)
{
    SqSplit r = { 0, -1, -1, 0, 0, 0, 0 };
    if (S < p.min_support || S == 0) return r;
    uint32_t best = SQ_NO_KEY;
    for (int32_t c = 0; c < S; c++) { const uint32_t k = sq_cost_key(sq_cost(mat, stride, S, c), c); if (k < best) best = k; }
    r.zygosity = 1; r.c0 = (int32_t)(best & 255u); r.cost1 = r.cost2 = (int64_t)(best >> 8); r.n0 = S;
    uint32_t key = SQ_NO_KEY;
    for (int32_t c0 = 0; c0 < S; c0++)
        for (int32_t c1 = c0 + 1; c1 < S; c1++) {
            int32_t n0, cost2;
            sq_pair_eval(mat, stride, S, c0, c1, n0, cost2);
            if (!sq_admissible(p, S, n0, mat[c1 * stride + c0], r.cost1, cost2)) continue;
            const uint32_t k = sq_pair_key(cost2, c0, c1);
            if (k < key) key = k;
        }
    if (key == SQ_NO_KEY) return r;
    r.zygosity = 2; r.c0 = (int32_t)((key >> 7) & 127u); r.c1 = (int32_t)(key & 127u); r.cost2 = (int64_t)(key >> 14);
    int32_t cost2;
    sq_pair_eval(mat, stride, S, r.c0, r.c1, r.n0, cost2);
    r.n1 = S - r.n0;
    return r;
}

// where member u of the list goes under split r: allele 0's members keep list order in front, allele 1's follow in list order.  before0 = the
// members in front of u that belong to c0 (the kernel: a ballot's bits below the lane plus the chunks before).  Zygosity 0 and 1 keep the list.
BA_HD int32_t sq_place(const SqSplit &r, int32_t u, bool first, int32_t before0) { return r.zygosity < 2 ? u : first ? before0 : r.n0 + (u - before0); }
