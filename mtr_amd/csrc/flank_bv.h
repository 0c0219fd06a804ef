// flank_bv.h — approximate matching of ONE short pattern against ONE read (or a window of it) in Myers' bit-vector form, as one sequential
// function: the form the flank search runs one per lane (flank_search.hip.inc: 64 reads per wavefront, the pattern's masks wave-uniform).
// Plain C++, nothing of HIP: the same functions compile into the gfx950 kernels and into a host program (tests/flank_bv_check.cpp).
//
// The definition is include/mtr_hip.h's ("flank search"): for the text x[lo .. lo + L) and the pattern p[0 .. m), unit-cost edit distance ed,
//   d(e) = min over s <= e of ed(p, x[s .. e)), dist = min d(e), end = the smallest e with d(e) = dist, start = the largest s <= end with
//   ed(p, x[s .. end)) = dist - all three in the text's own coordinates (0 .. L).
//   forward     column e of the matrix D(i, e) = min(D(i-1, e-1) + [p[i-1] != x[e-1]], D(i-1, e) + 1, D(i, e-1) + 1), D(0, e) = 0, D(i, 0) = i is
//               held as its vertical deltas: bit i - 1 of Pv / Mv says D(i, e) - D(i - 1, e) is +1 / -1.  One column is the dozen word operations
//               of Myers (1999) in Hyyro's formulation; the bottom cell d(e) = D(m, e) follows the horizontal delta's bit m - 1.  Bits from m up
//               hold garbage that never travels down: every carry and every shift goes up.  `<` keeps the smallest end.
//   backward    the reversed pattern against x[end - 1], x[end - 2], ... with row 0 costing j (a 1 shifted into the positive horizontal delta each
//               column): the bottom cell of column j is ed(p, x[end - j .. end)), and the first j at which it equals dist is the largest start.
//               It exists at some j <= min(end, m + dist); a scan that does not find it there did not get a consistent dist: start = -1.
//   masks       eq[c] has bit i set where p[i] is base c; rev[c] the same for the reversed pattern (fbv_masks: the host makes both).
//   text        2 bits per base, first base in the top bits of word 0 (the device layout).  How a word is had is the Load type's business:
//               ld(w) -> word w.  One load per 16 bases, issued a word ahead of its use, and never of a word the window does not touch.
// W is the word: uint32_t for m <= 32, uint64_t for m <= 64.
#pragma once
#include "mtr_common.h"

#define FBV_HD static inline __host__ __device__ __attribute__((always_inline))
#define FBV_MAX_M 64

struct FbvHit { int dist, start, end; };
template <class W> struct FbvMasks { W a, c, g, t; };

// the masks of codes[0 .. m) (0..3 each), read forwards (reversed = 0) or backwards
template <class W>
FBV_HD FbvMasks<W> fbv_masks(const uint8_t *codes, int m, int reversed)
{
    W v[4] = { 0, 0, 0, 0 };
    for (int i = 0; i < m && i < (int)(8 * sizeof(W)); i++) v[codes[reversed ? m - 1 - i : i] & 3] |= (W)1 << i;
    const FbvMasks<W> r = { v[0], v[1], v[2], v[3] };
    return r;
}
// (no array is indexed by a variable: on the GPU that would be a stack, and this runs one per lane.  The four are taken by VALUE before they are
// chosen among: `cond ? q.t : q.g` on the members themselves is a choice between two ADDRESSES, which keeps the struct in memory - hipcc put it
// into LDS, 32 bytes per lane.)
template <class W>
FBV_HD W fbv_pick(const FbvMasks<W> &q, int c)
{
    const W a = q.a, cc = q.c, g = q.g, t = q.t;
    const W lo = (c & 1) ? cc : a, hi = (c & 1) ? t : g;
    return (c & 2) ? hi : lo;
}

// one column: the text's base has the match mask eq; in_h = 1 shifts a +1 into row 0's horizontal delta (the anchored scan), 0 a 0 (the search)
template <class W>
FBV_HD void fbv_column(W eq, W top, W in_h, W &pv, W &mv, int &score)
{
    const W xv = eq | mv;
    const W xh = (((eq & pv) + pv) ^ pv) | eq;
    W ph = mv | ~(xh | pv);
    W mh = pv & xh;
    score += (ph & top) ? 1 : (mh & top) ? -1 : 0;
    ph = (W)(ph << 1) | in_h;
    mh = (W)(mh << 1);
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

template <class W, class Load>
FBV_HD FbvHit fbv_search(const Load &ld, int L, const FbvMasks<W> &eq, const FbvMasks<W> &rev, int m, int lo = 0)
{
    const W top = (W)1 << (m - 1);
    W pv = ~(W)0, mv = 0;
    int score = m, best = m, end = 0;
    // Word by word, the bases of a word in a loop of their own: the word in hand is w, the next one is already on its way and is waited for
    // only when it becomes the word in hand (a lane would wait for a load once per 16 columns otherwise, and a slot's groups are too few
    // wavefronts to hide that).
    if (L > 0) {
        const int first = lo >> 4, last = (lo + L - 1) >> 4;     // the words the window touches
        uint32_t wn = ld(first);
        for (int k = first; k <= last; k++) {
            const uint32_t w = wn;
            if (k < last) wn = ld(k + 1);
            const int p0 = k == first ? lo : k << 4, p1 = k == last ? lo + L : (k + 1) << 4;      // (a window begins and ends inside a word)
            for (int p = p0; p < p1; p++) {
                fbv_column<W>(fbv_pick(eq, (int)((w >> (30 - 2 * (p & 15))) & 3u)), top, (W)0, pv, mv, score);
                if (score < best) { best = score; end = p + 1 - lo; }
            }
        }
    }
    // the anchored scan back from x[end - 1]
    FbvHit h = { best, -1, end };
    pv = ~(W)0; mv = 0; score = m;
    if (score == best) { h.start = end; return h; }
    const int reach = end < m + best ? end : m + best;           // (>= 1: score != best means end >= 1)
    const int hi = lo + end - 1, low = lo + end - reach;         // the text positions it may visit, downwards
    uint32_t wn = ld(hi >> 4);
    for (int k = hi >> 4; k >= (low >> 4) && h.start < 0; k--) {
        const uint32_t w = wn;
        if (k > (low >> 4)) wn = ld(k - 1);
        const int p1 = k == (hi >> 4) ? hi : (k << 4) + 15, p0 = k == (low >> 4) ? low : k << 4;
        for (int p = p1; p >= p0; p--) {
            fbv_column<W>(fbv_pick(rev, (int)((w >> (30 - 2 * (p & 15))) & 3u)), top, (W)1, pv, mv, score);
            if (score == best) { h.start = p - lo; break; }
        }
    }
    return h;
}
