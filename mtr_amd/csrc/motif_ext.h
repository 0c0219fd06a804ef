// motif_ext.h — the ANCHORED EXTENSION of a read's window against ONE short motif as one sequential function: the form the partial genotype runs
// one per lane (partial.hip.inc: 64 tasks of one variant per wavefront, the motif wave-uniform; partial_catalog.hip.inc: 64 tasks of any loci, the
// motif, its length and the direction the lane's own, through motif_ext_rows<UB, false> directly).  Plain C++, nothing of HIP: the same function
// compiles into the gfx950 kernels and into host programs (tests/motif_ext_check.cpp, tests/motif_ext_masked_check.cpp).
//
// The definition is include/mtr_hip.h's ("partial genotype"): motif_dp.h's wrap-around recurrence started at the flank's boundary and WITHOUT the
// zero floor - a path begins in row 0 and nowhere else, so the best cell says how far the repeat runs from the flank - with what a traceback would
// count carried forward instead of cells stored.
//   rows        row i stands for y[i - 1]: x[lo + i - 1] going forward, x[hi - i] going backward; n = hi - lo rows.  The word in hand is
//               reloaded only at a word's edge (a window begins inside a word; a backward window walks the words downwards), and no word
//               outside [lo >> 4, (hi - 1) >> 4] is ever loaded.
//   cells       H(i, j) = max(sub, left, up), sub = H(i - 1, j - 1) + (G on a match, else -MM), left = H(i, j - 1) - D (none in column 1), up =
//               H(i - 1, j) - D; H(i - 1, 0) = H(i - 1, U); row 0 is zeros in every column (the phase at the flank is free).
//   carried     C (motif bases consumed) and T (matches) of the predecessor - the FIRST of sub, left, up that attains H, the traceback's order -
//               plus 1 to C for sub and left, plus 1 to T for a matching sub.  The previous row of H, C and T is three arrays of UB registers
//               (UB = the bucket: 4, 8, 16, 32); the loop over the columns is unrolled over UB, so every index is a constant, and cut at U
//               WITHOUT a branch: a motif that fills its bucket (U == UB) runs rows compiled without a cut; a shorter one computes all UB columns
//               and takes the best cell, the wrap (column U) and the row's maximum under the mask j < U (wave-uniform in partial.hip.inc, per lane in
//               partial_catalog.hip.inc: nothing here asks for either, and the masked rows are right for U == UB as well).  Columns >= U read
//               columns < U and are read by none of them.  (Cut by branches - motif_dp_forward's way - the three arrays' registers were moved
//               around at every cut: 67 instructions per cell built, about 40 of them moves.)  The motif is 2 bits per base in a 64-bit
//               value, m[j] at bits 2j: the host hands the backward variants reversed.
//   best cell   the first strict maximum over the rows >= 1 in row-major order, if positive: the loops ARE row-major, `>` against a best that
//               starts at 0 is the whole rule.  Its column is not needed: only its row, H, C and T.
//   early exit  a row's maximum grows by at most G per row, so once max_j H(i, j) + G * (n - i) <= best no later cell can be a strict maximum:
//               the lane stops.  Exact; looked at once per word.
#pragma once
#include "motif_dp.h"

struct MotifExt { int ext_len, motif_bases, matches, score; };     // bi, C, T and H of the best cell; zeros without a positive cell

// ld(w): word w of the read in the device layout (2 bits per base, first base in the top bits of word 0); 0 <= lo <= hi; back: 0 forward from lo,
// 1 backward from hi; 1 <= U <= UB.  FULL: U == UB, known when compiled - nothing to cut
template <int UB, bool FULL, class Load>
MDP_HD MotifExt motif_ext_rows(const Load &ld, int lo, int hi, int back, uint64_t mot, int U, int G, int MM, int D)
{
    static_assert(UB >= 1 && UB <= MDP_MAX_U, "bucket");
    int H[UB], Cn[UB], T[UB];
    MDP_UNROLL
    for (int j = 0; j < UB; j++) { H[j] = 0; Cn[j] = 0; T[j] = 0; }
    int wH = 0, wC = 0, wT = 0;                                  // column U of the previous row
    int bv = 0, bi = 0, bc = 0, bt = 0;
    const int n = hi - lo, edge = back ? 15 : 0, last = back ? 0 : 15;
    uint32_t w = 0;
    for (int i = 1; i <= n; i++) {
        const int p = back ? hi - i : lo + i - 1, b = p & 15;
        if (b == edge || i == 1) w = ld(p >> 4);
        const int xi = (int)((w >> (30 - 2 * b)) & 3u);
        int dH = wH, dC = wC, dT = wT, lH = 0, lC = 0, lT = 0;
    MDP_UNROLL
        for (int j = 0; j < UB; j++) {
            const bool on = FULL || j < U;                       // (wave-uniform where the wavefront shares a motif; a lane's own otherwise)
            const int mj = (int)((mot >> (2 * j)) & 3u);
            const bool m = xi == mj;
            const int uH = H[j], uC = Cn[j], uT = T[j];
            int h = dH + (m ? G : -MM), c = dC + 1, t = dT + (m ? 1 : 0);
            if (j > 0) {
                const int l = lH - D;
                const bool take = l > h;
                h = take ? l : h; c = take ? lC + 1 : c; t = take ? lT : t;
            }
            const int u = uH - D;
            const bool take = u > h;
            h = take ? u : h; c = take ? uC : c; t = take ? uT : t;
            const bool better = on && h > bv;
            bv = better ? h : bv; bi = better ? i : bi; bc = better ? c : bc; bt = better ? t : bt;
            dH = uH; dC = uC; dT = uT;
            H[j] = h; Cn[j] = c; T[j] = t;
            lH = h; lC = c; lT = t;
            if (!FULL) { const bool end = j == U - 1; wH = end ? h : wH; wC = end ? c : wC; wT = end ? t : wT; }
        }
        if (FULL) { wH = lH; wC = lC; wT = lT; }
        if (b == last) {
            int mx = H[0];
    MDP_UNROLL
            for (int j = 1; j < UB; j++) mx = (FULL || j < U) && H[j] > mx ? H[j] : mx;
            if (mx + G * (n - i) <= bv) break;
        }
    }
    const MotifExt r = { bi, bc, bt, bv };
    return r;
}

template <int UB, class Load>
MDP_HD MotifExt motif_ext(const Load &ld, int lo, int hi, int back, uint64_t mot, int U, int G, int MM, int D)
{
    return U == UB ? motif_ext_rows<UB, true>(ld, lo, hi, back, mot, U, G, MM, D) : motif_ext_rows<UB, false>(ld, lo, hi, back, mot, U, G, MM, D);
}
