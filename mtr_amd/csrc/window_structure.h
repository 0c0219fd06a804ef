// window_structure.h — the MOTIF STRUCTURE of one oriented window: its global alignment to an ordered list of motifs, each repeated zero or more
// whole times, as one sequential function with everything a traceback would count carried forward.  The window-structure call runs it one window
// per lane (window_structure.hip.inc: mtr_k_ws_lanes, the structure the lane's own).  Plain C++, nothing of HIP: the same function compiles into
// the gfx950 kernels and into a host program (tests/window_structure_check.cpp).  The checks of the call's host arguments are at the end.
//
// The definition is include/mtr_hip.h's ("window structure").  How it is computed here:
//   structure   one lane's own: the motif codes 2 bits per column in a 64-bit value (m[c] at bits 2c), first(s) and last(s) as 32-bit masks over
//               the columns, seg(c) 2 bits per column.  W <= UB columns; the bucket's columns beyond W are computed and read by none below W.
//   rows        row i stands for y[i - 1]; row 0 runs through the same body with the row before it at minus infinity (WS_NEG), which leaves it
//               its lefts.  The window's bytes come 8 at a time: ld(k) is the aligned 8-byte word k of the window, word 0 the one that holds y[0]
//               at byte r (r = the window's address mod 8); no word outside 0 .. (r + n - 1) >> 3 is asked for.
//   a cell      H and the packed entry, copies and matches: 16 bits per segment, two segments in 32 bits (narrow), four in 64 (WIDE).  The
//               previous row is four arrays of UB registers; the loop over the columns is unrolled over UB, so every index is a constant, and
//               what a column is - a first, a last, its segment, beyond W - is the lane's masks, never a branch (motif_ext.h says why).
//   sweep 1     columns ascending: sub (the predecessors in the definition's order), up, left.  A first column's predecessors from outside its
//               segment - last(s - 1) .. last(0), START - are ONE running best per row (o: of row i - 1, for the subs; q: of row i, for the lefts):
//               each last column enters it with >=, so the higher segment wins a tie as the order asks.  The segment's own wrap of row i - 1
//               (w[s], kept per segment when its last column is computed) comes after them: taken when strictly greater.
//   sweep 2     columns ascending again: a first column takes w[s] of row i (final: sweep 2 never changes a last column) minus D, every other
//               column its left neighbour minus D, when strictly greater - the wrap's left and its run-on, and nothing else can fire.
//   the end     q after row n is the best of last(S - 1) .. last(0), START in that order.
#pragma once
#include <cstdint>
#include "motif_dp.h"

#define WS_MAX_SEGMENTS 4
#define WS_MAX_WINDOW 16384
#define WS_MAX_W_NARROW 32                  // S <= 2
#define WS_MAX_W_WIDE 16                    // S <= 4
#define WS_NEG (-(1 << 28))                 // minus infinity: below every cell, and D * WS_MAX_WINDOW below it still does not wrap

struct WsStruct { uint64_t mot, seg; uint32_t first, last; int32_t W, S; };        // one structure as a lane carries it
struct WsRaw { int32_t score; uint32_t pad; uint64_t entry, copies, matches; };     // the end's H and carried fields, 16 bits per segment

template <bool WIDE> struct WsCnt { typedef uint32_t type; };
template <> struct WsCnt<true> { typedef uint64_t type; };

// the entry field of segment sg (at bit sh = 16 * sg) set to v
template <class P> MDP_HD P ws_set_entry(P e, int sh, int v) { return (e & ~((P)0xffff << sh)) | ((P)(v & 0xffff) << sh); }

// ld(k): see "rows"; 0 <= r < 8; 0 <= n <= WS_MAX_WINDOW; 1 <= W <= UB; S <= 2, or WIDE and S <= 4
template <int UB, bool WIDE, class Load>
MDP_HD WsRaw ws_rows(const Load &ld, int r, int n, const WsStruct &st, int G, int MM, int D)
{
    static_assert(UB >= 1 && UB <= 32 && (!WIDE || UB <= 16), "bucket");
    typedef typename WsCnt<WIDE>::type P;
    constexpr int NS = WIDE ? 4 : 2;
    const uint64_t mot = st.mot, segb = st.seg;
    const uint32_t firstm = st.first, lastm = st.last;
    int H[UB]; P E[UB], Cn[UB], M[UB];
    MDP_UNROLL
    for (int c = 0; c < UB; c++) { H[c] = WS_NEG; E[c] = 0; Cn[c] = 0; M[c] = 0; }
    int wH[NS]; P wE[NS], wC[NS], wM[NS];                        // last(s) of the row in hand, s = 0 .. NS - 1
    MDP_UNROLL
    for (int s = 0; s < NS; s++) { wH[s] = WS_NEG; wE[s] = 0; wC[s] = 0; wM[s] = 0; }
    int qH = 0; P qE = 0, qC = 0, qM = 0;
    uint64_t word = 0;
    for (int i = 0; i <= n; i++) {
        int yi = 0;
        if (i >= 1) {
            const int p = r + i - 1;
            if (i == 1) word = ld(p >> 3) >> (8 * (p & 7));
            else if ((p & 7) == 0) word = ld(p >> 3);
            yi = (int)(word & 0xffu);
            word >>= 8;
        }
        int oH = i >= 1 ? -D * (i - 1) : WS_NEG; P oE = 0, oC = 0, oM = 0;      // START of row i - 1 ..
        qH = -D * i; qE = 0; qC = 0; qM = 0;                                    // .. and of row i
        int dH = WS_NEG, lH = WS_NEG; P dE = 0, dC = 0, dM = 0, lE = 0, lC = 0, lM = 0;
        // ---- sweep 1 ----
    MDP_UNROLL
        for (int c = 0; c < UB; c++) {
            const bool isf = (firstm >> c) & 1u, isl = (lastm >> c) & 1u;
            const int sg = (int)((segb >> (2 * c)) & 3u), sh = 16 * sg;
            const P one = (P)1 << sh;
            const bool mt = yi == (int)((mot >> (2 * c)) & 3u);
            int ownH = wH[0]; P ownE = wE[0], ownC = wC[0], ownM = wM[0];
    MDP_UNROLL
            for (int s = 1; s < NS; s++) { const bool k = sg == s; ownH = k ? wH[s] : ownH; ownE = k ? wE[s] : ownE; ownC = k ? wC[s] : ownC; ownM = k ? wM[s] : ownM; }
            const int uH = H[c]; const P uE = E[c], uC = Cn[c], uM = M[c];
            // sub: from outside before the own wrap; inside a segment from the column before
            const bool own = ownH > oH;
            const int pH = isf ? (own ? ownH : oH) : dH;
            const P pE = isf ? (own ? ownE : ws_set_entry<P>(oE, sh, i - 1)) : dE;
            const P pC = isf ? (own ? ownC : oC) : dC, pM = isf ? (own ? ownM : oM) : dM;
            int h = pH + (mt ? G : -MM);
            P e = pE, cn = pC + (isl ? one : (P)0), m = pM + (mt ? one : (P)0);
            // up
            const int u = uH - D;
            const bool tu = u > h;
            h = tu ? u : h; e = tu ? uE : e; cn = tu ? uC : cn; m = tu ? uM : m;
            // left: from outside (the wrap's left is sweep 2's), or from the column before
            const int l = (isf ? qH : lH) - D;
            const bool tl = l > h;
            h = tl ? l : h; e = tl ? (isf ? ws_set_entry<P>(qE, sh, i) : lE) : e; cn = tl ? (isf ? qC : lC) + (isl ? one : (P)0) : cn; m = tl ? (isf ? qM : lM) : m;
            dH = uH; dE = uE; dC = uC; dM = uM;
            H[c] = h; E[c] = e; Cn[c] = cn; M[c] = m;
            lH = h; lE = e; lC = cn; lM = m;
            // a last column: into the two outside bests (the higher segment wins a tie), and the segment's wrap
            const bool to = isl && uH >= oH, tq = isl && h >= qH;
            oH = to ? uH : oH; oE = to ? uE : oE; oC = to ? uC : oC; oM = to ? uM : oM;
            qH = tq ? h : qH; qE = tq ? e : qE; qC = tq ? cn : qC; qM = tq ? m : qM;
    MDP_UNROLL
            for (int s = 0; s < NS; s++) { const bool k = isl && sg == s; wH[s] = k ? h : wH[s]; wE[s] = k ? e : wE[s]; wC[s] = k ? cn : wC[s]; wM[s] = k ? m : wM[s]; }
        }
        // ---- sweep 2: the wrap's left and its run-on (a last column is never reached: once round a segment costs U * D) ----
        lH = WS_NEG; lE = 0; lC = 0; lM = 0;
    MDP_UNROLL
        for (int c = 0; c < UB; c++) {
            const bool isf = (firstm >> c) & 1u;
            const int sg = (int)((segb >> (2 * c)) & 3u);
            int fH = wH[0]; P fE = wE[0], fC = wC[0], fM = wM[0];
    MDP_UNROLL
            for (int s = 1; s < NS; s++) { const bool k = sg == s; fH = k ? wH[s] : fH; fE = k ? wE[s] : fE; fC = k ? wC[s] : fC; fM = k ? wM[s] : fM; }
            const int l = (isf ? fH : lH) - D;
            const bool t = l > H[c];
            H[c] = t ? l : H[c]; E[c] = t ? (isf ? fE : lE) : E[c]; Cn[c] = t ? (isf ? fC : lC) : Cn[c]; M[c] = t ? (isf ? fM : lM) : M[c];
            lH = H[c]; lE = E[c]; lC = Cn[c]; lM = M[c];
        }
    }
    const WsRaw out = { qH, 0u, (uint64_t)qE, (uint64_t)qC, (uint64_t)qM };
    return out;
}

// the spans of the definition's `seg` column out of the end's carried fields: start, end, copies, matches per segment, zeros from S on
MDP_HD void ws_spans(const WsRaw &raw, int n, int S, int32_t *seg16)
{
    int nxt = n;
    for (int s = WS_MAX_SEGMENTS - 1; s >= 0; s--) {
        const int cp = (int)((raw.copies >> (16 * s)) & 0xffffu), mt = (int)((raw.matches >> (16 * s)) & 0xffffu), en = (int)((raw.entry >> (16 * s)) & 0xffffu);
        int32_t *o = seg16 + 4 * s;
        if (s >= S) { o[0] = o[1] = o[2] = o[3] = 0; continue; }
        if (cp > 0) { o[0] = en; o[1] = nxt; o[2] = cp; o[3] = mt; nxt = en; }
        else { o[0] = nxt; o[1] = nxt; o[2] = 0; o[3] = 0; }
    }
}
MDP_HD int ws_matches(const WsRaw &raw) { int t = 0; for (int s = 0; s < WS_MAX_SEGMENTS; s++) t += (int)((raw.matches >> (16 * s)) & 0xffffu); return t; }
// the bucket of W columns (8, 16 or 32) and whether S segments need the wide counters
MDP_HD int ws_bucket(int W) { return W <= 8 ? 8 : W <= 16 ? 16 : 32; }
MDP_HD bool ws_wide(int S) { return S > 2; }
MDP_HD bool ws_limit_ok(int S, int64_t W) { return S >= 1 && W >= 1 && ((S <= 2 && W <= WS_MAX_W_NARROW) || (S <= WS_MAX_SEGMENTS && W <= WS_MAX_W_WIDE)); }
