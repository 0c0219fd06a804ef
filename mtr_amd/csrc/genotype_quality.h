// genotype_quality.h — the genotype quality's arithmetic: the quality-weighted banded score s(e, a) of one supporting read's oriented window
// against one allele's sequence, what an entry makes of its two scores, and the reduction of a locus' scores to genotype likelihoods.  Plain
// C++, nothing of HIP: the same functions compile into the gfx950 kernels (genotype_quality.hip.inc) and into a host program
// (tests/genotype_quality_check.cpp), which holds them to a full matrix and to a naive loop.
//
// The definition is include/mtr_hip.h's ("genotype quality").  The band (ba_band - part of the definition, as in the consensus), the
// anti-diagonal schedule - pairs of diagonals (E, O), one neighbour value per step - and the weights baq_weight and baq_gap are
// banded_align.h's; the cell differs from ba_cell in its costs alone and keeps no direction: nothing is kept per cell.
//   costs       of cell (i, j): a substitution costs omega[i-1] = baq_weight(Q[i-1]), a step up (the read's base i-1 against nothing)
//               min(omega[i-1], gap_cap), a step left (the allele's base j-1 against the read's boundary i) min(gamma(i), gap_cap).  All three
//               are derived in the step from the read's quality bytes Q[i-1] and Q[i] - two byte loads beside the two base loads and a few
//               clamps - rather than prepared as three bytes per base by a kernel of its own: prepared costs would be three loads a cell
//               instead of two, a buffer of three times the windows' size and one more launch, to save the clamps.  Q == NULL: every
//               quality is qual_cap and nothing is loaded
//   values      a score is at most 32 768 steps of at most 93: below BA_INF = 2^29, which stays BA_INF through the cell's clamp
#pragma once
#include "banded_align.h"

#define GQ_MAX_READ_CAP (1 << 20)  // read_cap's limit: 2^31 - 1 entries of at most 2^20 + 3 stay inside int64 by far
#define GQ_NO_GT 255

struct GqParams { int32_t band_extra, qual_cap, gap_cap, read_cap; };

// ---- the score ------------------------------------------------------------------------------------------------------------------------------
BA_HD int32_t gq_min(int32_t a, int32_t b) { return a < b ? a : b; }
// the weight of base k of a window whose qualities are Q (NULL: every quality is the cap)
BA_HD int32_t gq_omega(const uint8_t *Q, int32_t k, int32_t cap) { return Q ? baq_weight(Q[k], cap) : cap; }
// the gap weight at boundary i (0 .. n): baq_gap, with the NULL column
BA_HD int32_t gq_gamma(const uint8_t *Q, int32_t n, int32_t i, int32_t cap) { return Q ? baq_gap(Q, n, i, cap) : n == 0 ? 1 : cap; }

// one cell from its three inputs (BA_INF: none), each before its own cost is added
BA_HD int32_t gq_cell(int32_t diag, int32_t up, int32_t left, int32_t c_sub, int32_t c_up, int32_t c_left)
{
    const int32_t best = gq_min(diag + c_sub, gq_min(up + c_up, left + c_left));
    return best < BA_INF ? best : BA_INF;
}

// the cell of band diagonal e on anti-diagonal s ((s - dlo - e) even) from the running values, as ba_step_cell: W, Q the read's window and its
// qualities, C the allele's sequence
BA_HD int32_t gq_step_cell(int32_t s, int32_t e, int32_t n, int32_t m, const BaBand &b, int32_t diag, int32_t up, int32_t left, const uint8_t *W, const uint8_t *Q,
                           const uint8_t *C, const GqParams &p)
{
    const int32_t d = b.dlo + e, i2 = s - d, j2 = s + d;
    if (d > b.dhi || i2 < 0 || j2 < 0 || i2 > 2 * n || j2 > 2 * m) return BA_INF;
    if (s == 0) return 0;
    const int32_t i = i2 >> 1, j = j2 >> 1;
    const int32_t omega = i >= 1 ? gq_omega(Q, i - 1, p.qual_cap) : 1;           // (row 0 has neither a diagonal nor an upper input: the cost does not matter)
    const int32_t c_sub = i >= 1 && j >= 1 && W[i - 1] == C[j - 1] ? 0 : omega;
    return gq_cell(diag, up, left, c_sub, gq_min(omega, p.gap_cap), gq_min(gq_gamma(Q, n, i, p.qual_cap), p.gap_cap));
}

// One step of pair q on anti-diagonal s, whichever parity the task's band gives it (sq_step's shape): the pair's running values (E, O), `below`
// = O of pair q - 1, `above` = E of pair q + 1 (BA_INF at the band's ends)
BA_HD void gq_step(int32_t s, int32_t q, int32_t n, int32_t m, const BaBand &b, int32_t &E, int32_t &O, int32_t below, int32_t above, const uint8_t *W, const uint8_t *Q,
                   const uint8_t *C, const GqParams &p)
{
    const int par = (s - b.dlo) & 1;
    const int32_t v = gq_step_cell(s, 2 * q + par, n, m, b, par ? O : E, par ? above : O, par ? E : below, W, Q, C, p);
    if (par) O = v; else E = v;
}
// One step of the CPL pairs lane * CPL .. lane * CPL + CPL - 1 that ONE lane of a whole wavefront holds (the <1, CPL> shapes; the task's parity
// is the wavefront's).  `neighbour` is the one value from another lane: on an even step O[CPL - 1] of lane - 1, on an odd step E[0] of lane + 1
// (BA_INF at the wavefront's ends); the other neighbours are the lane's own registers.
template <int CPL>
BA_HD void gq_step_lane(int32_t s, int32_t lane, int32_t n, int32_t m, const BaBand &b, int32_t *E, int32_t *O, int32_t neighbour, const uint8_t *W, const uint8_t *Q,
                        const uint8_t *C, const GqParams &p)
{
    if (((s - b.dlo) & 1) == 0) {
        for (int k = 0; k < CPL; k++) E[k] = gq_step_cell(s, 2 * (lane * CPL + k), n, m, b, E[k], O[k], k > 0 ? O[k > 0 ? k - 1 : 0] : neighbour, W, Q, C, p);
    } else {
        for (int k = 0; k < CPL; k++) O[k] = gq_step_cell(s, 2 * (lane * CPL + k) + 1, n, m, b, O[k], k + 1 < CPL ? E[k + 1 < CPL ? k + 1 : 0] : neighbour, E[k], W, Q, C, p);
    }
}
// which band diagonal holds D(n, m) after step n + m: pair e >> 1, its O if e is odd, else its E
BA_HD int32_t gq_end_diagonal(int32_t n, int32_t m, const BaBand &b) { return m - n - b.dlo; }

// the whole fill in the kernels' schedule by ONE thread, for a pair that is not ba_skipped: E, O hold (ba_width + 1) / 2 values each (at most
// 128).  Returns s(e, a).  The kernels run the same steps with pair q in lane q (a row of 16, half a wavefront, or its 64) or in lane q / 2.
BA_HD int32_t gq_fill(int32_t n, int32_t m, const uint8_t *W, const uint8_t *Q, const uint8_t *C, const GqParams &p, int32_t *E, int32_t *O)
{
    const BaBand b = ba_band(n, m, p.band_extra);
    const int32_t pairs = (ba_width(b) + 1) >> 1;
    for (int32_t q = 0; q < pairs; q++) E[q] = O[q] = BA_INF;
    for (int32_t s = 0; s <= n + m; s++)
        for (int32_t q = 0; q < pairs; q++)                                     // (a step writes one of E, O and reads the neighbours' other one: any order of q)
            gq_step(s, q, n, m, b, E[q], O[q], q > 0 ? O[q - 1] : BA_INF, q + 1 < pairs ? E[q + 1] : BA_INF, W, Q, C, p);
    const int32_t e = gq_end_diagonal(n, m, b);
    return (e & 1) ? O[e >> 1] : E[e >> 1];
}

// ---- an entry ---------------------------------------------------------------------------------------------------------------------------------
// best and margin of an entry of a locus of zygosity z whose scores are s0, s1 (-1, -1: not scored) and whose allele column says `allele`
BA_HD void gq_entry(int z, int32_t s0, int32_t s1, int allele, uint8_t &best, int32_t &margin)
{
    best = (uint8_t)allele; margin = 0;
    if (s0 < 0) return;
    if (z == 1) best = 0;
    else if (z == 2) {
        if (s0 != s1) best = s0 < s1 ? 0 : 1;
        margin = s0 < s1 ? s1 - s0 : s0 - s1;
    }
}

// ---- a locus ------------------------------------------------------------------------------------------------------------------------------------
// T[d] = 10 log10(1 + 10^(-d / 10)) rounded, 0 from d = 10 on
BA_HD int32_t gq_T(int32_t d) { return d < 2 ? 3 : d < 4 ? 2 : d < 10 ? 1 : 0; }
// a read drawn from either allele with probability one half: x0, x1 are capped already
BA_HD int32_t gq_het(int32_t x0, int32_t x1)
{
    const int32_t d = x0 < x1 ? x1 - x0 : x0 - x1;
    return gq_min(x0, x1) + 3 - gq_T(gq_min(d, 10));
}

struct GqSums { int64_t r0, rh, r1; int32_t scored, unscored; };

// one entry's part of its locus' sums (z = 1: r0 alone; z = 0: nothing)
BA_HD void gq_add(GqSums &t, int z, int32_t s0, int32_t s1, int32_t read_cap)
{
    if (z == 0) return;
    if (s0 < 0) { t.unscored++; return; }
    t.scored++;
    const int32_t x0 = gq_min(s0, read_cap);
    t.r0 += x0;
    if (z == 2) { const int32_t x1 = gq_min(s1, read_cap); t.rh += gq_het(x0, x1); t.r1 += x1; }
}
BA_HD void gq_merge(GqSums &t, const GqSums &o) { t.r0 += o.r0; t.rh += o.rh; t.r1 += o.r1; t.scored += o.scored; t.unscored += o.unscored; }

// the locus' columns from its sums: raw and pl in the order 0/0, 0/1, 1/1
BA_HD void gq_finish(int z, const GqSums &t, int64_t *raw, int64_t *pl, uint8_t &gt, int64_t &gq)
{
    if (z == 2) {
        raw[0] = t.r0; raw[1] = t.rh; raw[2] = t.r1;
        const int g = raw[1] <= raw[0] && raw[1] <= raw[2] ? 1 : raw[0] <= raw[2] ? 0 : 2;          // ties in the order 0/1, 0/0, 1/1
        for (int k = 0; k < 3; k++) pl[k] = raw[k] - raw[g];
        const int64_t a = pl[(g + 1) % 3], b = pl[(g + 2) % 3];
        gt = (uint8_t)g; gq = a < b ? a : b;
    } else {
        raw[0] = z == 1 ? t.r0 : -1; pl[0] = z == 1 ? 0 : -1;
        raw[1] = raw[2] = pl[1] = pl[2] = -1;
        gt = z == 1 ? 0 : GQ_NO_GT; gq = -1;
    }
}
