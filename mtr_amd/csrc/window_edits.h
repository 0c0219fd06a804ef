// window_edits.h — the EDITS of one oriented window: the path of its window structure read out step by step, as two sequential functions.  Plain
// C++, nothing of HIP: the same functions compile into the gfx950 kernels (window_edits.hip.inc) and into a host program
// (tests/window_edits_check.cpp).  The definition is include/mtr_hip.h's ("window edits"); the cells are window_structure.h's, unchanged.
//   we_rows     ws_rows' rows once more - the same cells, the same carried fields, the same order of every comparison, held to ws_rows bit for
//               bit by the host program - and per row ONE record of what every column decided, handed to a sink when the row is final:
//                 kinds   2 bits a column after sweep 2: WE_SUB a matching sub, WE_SUBX a mismatching one, WE_UP, WE_LEFT (sweep 2's override
//                         is a left).  That a sub matched is stored, so the walk that only counts never looks at the window
//                 ids     3 bits a segment: the predecessor of first(s)' winning sub or left from OUTSIDE its row of columns - t for last(t)
//                         (t == s is the wrap), WE_START for START.  The outside bests o and q are one running value per row: which last column
//                         or START holds them travels with them (oI, qI), because nothing else can recover it.  qI after row n is the end
//               The record as 32-bit words (we_pack / we_unpack): bucket 8: kinds | ids << 16, one word; 16: kinds, ids, two; 32: kinds low,
//               kinds high, ids, three.  Every row is whole words of its own: no two rows share a word.
//   we_walk     from the end back to START by the stored decisions, one row record per step (asked for again only when the row changes).  It
//               counts the edits and, from the steps alone, copies, matches and entries per segment: equal to what we_rows carried forward,
//               or the stored decisions are not the path.  With EMIT it writes each edit's row, the last first, down from the end of the
//               window's slice of the list, so that the list reads in path order; the copy index of a step is the segment's counted copies
//               minus the landings on first(s) the walk has already passed, minus one.  A record that cannot be (a step out of row 0 upward,
//               a column below 0, lefts round and round, more edits than were counted) ends the walk with `bad` set: nothing is read or
//               written outside the window's rows and its slice.
#pragma once
#include "window_structure.h"

#define WE_SUB 0
#define WE_UP 1
#define WE_LEFT 2
#define WE_SUBX 3
#define WE_START 4                          // among the ids: START (the segments are 0 .. 3)
#define WE_FIELDS 6                         // an edit's row: pos, segment, copy, column, kind, base

// On the device the structure's words are made opaque once per row: what a column is - a first, a last, its segment - is then worked out where it is
// used, in the row.  Left visible, the tests are hoisted out of the row loop as lane masks in scalar registers, hundreds of them, spilled to VGPR
// lanes.  A column's kind is made a number in a register the same way, where it is decided.
#if defined(__HIP_DEVICE_COMPILE__)
#define WE_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define WE_OPAQUE(x) ((void)0)
#endif

struct WeRow { uint64_t kinds; uint32_t ids; };
struct WeCount { uint64_t entry, copies, matches; int32_t edits, bad; };

MDP_HD int we_row_words(int UB) { return UB <= 8 ? 1 : UB <= 16 ? 2 : 3; }
// word k of the record (k < we_row_words(UB)) and back
MDP_HD uint32_t we_pack(int UB, const WeRow &r, int k)
{
    if (UB <= 8) return (uint32_t)r.kinds | (r.ids << 16);
    if (UB <= 16) return k == 0 ? (uint32_t)r.kinds : r.ids;
    return k == 0 ? (uint32_t)r.kinds : k == 1 ? (uint32_t)(r.kinds >> 32) : r.ids;
}
MDP_HD WeRow we_unpack(int UB, uint32_t w0, uint32_t w1, uint32_t w2)
{
    WeRow r;
    if (UB <= 8) { r.kinds = w0 & 0xffffu; r.ids = w0 >> 16; }
    else if (UB <= 16) { r.kinds = w0; r.ids = w1; }
    else { r.kinds = (uint64_t)w0 | ((uint64_t)w1 << 32); r.ids = w2; }
    return r;
}

// Where the previous row lives.  WeRowRegs: four register arrays of the bucket's width, the loops over the columns unrolled over UB (ws_rows' way).
// WeRowMem: four arrays in memory the caller gives (on the device LDS, column c of a lane at c * stride), the loops over the structure's W columns
// NOT unrolled: a few dozen registers and a page of code, for the two buckets whose unrolled form takes more than 256 registers.
template <int UB, class P> struct WeRowRegs {
    static constexpr bool rolled = false;
    int H[UB]; P E[UB], C[UB], M[UB];
    MDP_MEMBER int &h(int c) { return H[c]; }
    MDP_MEMBER P &e(int c) { return E[c]; }
    MDP_MEMBER P &cn(int c) { return C[c]; }
    MDP_MEMBER P &m(int c) { return M[c]; }
};
template <class P> struct WeRowMem {
    static constexpr bool rolled = true;
    int *H; P *E, *C, *M; int stride;
    MDP_MEMBER int &h(int c) { return H[c * stride]; }
    MDP_MEMBER P &e(int c) { return E[c * stride]; }
    MDP_MEMBER P &cn(int c) { return C[c * stride]; }
    MDP_MEMBER P &m(int c) { return M[c * stride]; }
};
#if defined(__clang__)
#define WE_STR_(x) #x
#define WE_STR(x) WE_STR_(x)
#define WE_UNROLL(n) _Pragma(WE_STR(unroll n))
#else
#define WE_UNROLL(n)
#endif

// ws_rows with the decisions kept: sink(i, record of row i) for i = 0 .. n in order; end_id = the end (a segment's last column, or WE_START)
template <int UB, bool WIDE, class Load, class Sink, class Rw>
MDP_HD WsRaw we_rows_in(Rw &row, const Load &ld, const Sink &sink, int r, int n, const WsStruct &st, int G, int MM, int D, int &end_id)
{
    static_assert(UB >= 1 && UB <= 32 && (!WIDE || UB <= 16), "bucket");
    typedef typename WsCnt<WIDE>::type P;
    constexpr int NS = WIDE ? 4 : 2;
    uint64_t mot = st.mot, segb = st.seg;
    uint32_t firstm = st.first, lastm = st.last;
    const int cols = Rw::rolled ? st.W : UB;
    WE_UNROLL((Rw::rolled ? 1 : UB))
    for (int c = 0; c < cols; c++) { row.h(c) = WS_NEG; row.e(c) = 0; row.cn(c) = 0; row.m(c) = 0; }
    int wH[NS]; P wE[NS], wC[NS], wM[NS];
    MDP_UNROLL
    for (int s = 0; s < NS; s++) { wH[s] = WS_NEG; wE[s] = 0; wC[s] = 0; wM[s] = 0; }
    int qH = 0, qI = WE_START; P qE = 0, qC = 0, qM = 0;
    uint64_t word = 0;
    for (int i = 0; i <= n; i++) {
        WE_OPAQUE(mot); WE_OPAQUE(segb); WE_OPAQUE(firstm); WE_OPAQUE(lastm);
        int yi = 0;
        if (i >= 1) {
            const int p = r + i - 1;
            if (i == 1) word = ld(p >> 3) >> (8 * (p & 7));
            else if ((p & 7) == 0) word = ld(p >> 3);
            yi = (int)(word & 0xffu);
            word >>= 8;
        }
        int oH = i >= 1 ? -D * (i - 1) : WS_NEG, oI = WE_START; P oE = 0, oC = 0, oM = 0;
        qH = -D * i; qI = WE_START; qE = 0; qC = 0; qM = 0;
        int dH = WS_NEG, lH = WS_NEG; P dE = 0, dC = 0, dM = 0, lE = 0, lC = 0, lM = 0;
        uint32_t klo = 0, khi = 0, ids = 0;                          // the kinds of columns 0 .. 15 and 16 .. 31
        // ---- sweep 1 ----
    WE_UNROLL((Rw::rolled ? 1 : UB))
        for (int c = 0; c < cols; c++) {
            const bool isf = (firstm >> c) & 1u, isl = (lastm >> c) & 1u;
            const int sg = (int)((segb >> (2 * c)) & 3u), sh = 16 * sg;
            const P one = (P)1 << sh;
            const bool mt = yi == (int)((mot >> (2 * c)) & 3u);
            int ownH = wH[0]; P ownE = wE[0], ownC = wC[0], ownM = wM[0];
    MDP_UNROLL
            for (int s = 1; s < NS; s++) { const bool k = sg == s; ownH = k ? wH[s] : ownH; ownE = k ? wE[s] : ownE; ownC = k ? wC[s] : ownC; ownM = k ? wM[s] : ownM; }
            const int uH = row.h(c); const P uE = row.e(c), uC = row.cn(c), uM = row.m(c);
            const bool own = ownH > oH;
            const int pH = isf ? (own ? ownH : oH) : dH;
            const P pE = isf ? (own ? ownE : ws_set_entry<P>(oE, sh, i - 1)) : dE;
            const P pC = isf ? (own ? ownC : oC) : dC, pM = isf ? (own ? ownM : oM) : dM;
            int h = pH + (mt ? G : -MM);
            P e = pE, cn = pC + (isl ? one : (P)0), m = pM + (mt ? one : (P)0);
            uint32_t id = own ? (uint32_t)sg : (uint32_t)oI;
            const int u = uH - D;
            const bool tu = u > h;
            h = tu ? u : h; e = tu ? uE : e; cn = tu ? uC : cn; m = tu ? uM : m;
            const int l = (isf ? qH : lH) - D;
            const bool tl = l > h;
            h = tl ? l : h; e = tl ? (isf ? ws_set_entry<P>(qE, sh, i) : lE) : e; cn = tl ? (isf ? qC : lC) + (isl ? one : (P)0) : cn; m = tl ? (isf ? qM : lM) : m;
            id = tl ? (uint32_t)qI : id;
            uint32_t kind = tl ? WE_LEFT : tu ? WE_UP : mt ? WE_SUB : WE_SUBX;
            WE_OPAQUE(kind);                                             // (a number in a register here, not three lane masks kept to the row's end)
            if (c < 16) klo |= kind << (2 * (c & 15)); else khi |= kind << (2 * (c & 15));
            ids |= isf ? id << (3 * sg) : 0u;
            dH = uH; dE = uE; dC = uC; dM = uM;
            row.h(c) = h; row.e(c) = e; row.cn(c) = cn; row.m(c) = m;
            lH = h; lE = e; lC = cn; lM = m;
            const bool to = isl && uH >= oH, tq = isl && h >= qH;
            oH = to ? uH : oH; oE = to ? uE : oE; oC = to ? uC : oC; oM = to ? uM : oM; oI = to ? sg : oI;
            qH = tq ? h : qH; qE = tq ? e : qE; qC = tq ? cn : qC; qM = tq ? m : qM; qI = tq ? sg : qI;
    MDP_UNROLL
            for (int s = 0; s < NS; s++) { const bool k = isl && sg == s; wH[s] = k ? h : wH[s]; wE[s] = k ? e : wE[s]; wC[s] = k ? cn : wC[s]; wM[s] = k ? m : wM[s]; }
        }
        // ---- sweep 2: an override is a left; at a first column it is the wrap's ----
        lH = WS_NEG; lE = 0; lC = 0; lM = 0;
    WE_UNROLL((Rw::rolled ? 1 : UB))
        for (int c = 0; c < cols; c++) {
            const bool isf = (firstm >> c) & 1u;
            const int sg = (int)((segb >> (2 * c)) & 3u);
            int fH = wH[0]; P fE = wE[0], fC = wC[0], fM = wM[0];
    MDP_UNROLL
            for (int s = 1; s < NS; s++) { const bool k = sg == s; fH = k ? wH[s] : fH; fE = k ? wE[s] : fE; fC = k ? wC[s] : fC; fM = k ? wM[s] : fM; }
            const int l = (isf ? fH : lH) - D;
            const int h0 = row.h(c); const P e0 = row.e(c), c0 = row.cn(c), m0 = row.m(c);
            const bool t = l > h0;
            lH = t ? l : h0; lE = t ? (isf ? fE : lE) : e0; lC = t ? (isf ? fC : lC) : c0; lM = t ? (isf ? fM : lM) : m0;
            row.h(c) = lH; row.e(c) = lE; row.cn(c) = lC; row.m(c) = lM;
            uint32_t over = t ? 1u : 0u;
            WE_OPAQUE(over);
            if (c < 16) klo = (klo & ~((over * 3u) << (2 * (c & 15)))) | ((over * WE_LEFT) << (2 * (c & 15)));
            else khi = (khi & ~((over * 3u) << (2 * (c & 15)))) | ((over * WE_LEFT) << (2 * (c & 15)));
            ids = t && isf ? (ids & ~(7u << (3 * sg))) | ((uint32_t)sg << (3 * sg)) : ids;
        }
        const WeRow rec = { (uint64_t)klo | ((uint64_t)khi << 32), ids };
        sink(i, rec);
    }
    end_id = qI;
    const WsRaw out = { qH, 0u, (uint64_t)qE, (uint64_t)qC, (uint64_t)qM };
    return out;
}

template <int UB, bool WIDE, class Load, class Sink>
MDP_HD WsRaw we_rows(const Load &ld, const Sink &sink, int r, int n, const WsStruct &st, int G, int MM, int D, int &end_id)
{
    WeRowRegs<UB, typename WsCnt<WIDE>::type> row;
    return we_rows_in<UB, WIDE>(row, ld, sink, r, n, st, G, MM, D, end_id);
}

// the column of last(t): the t-th set bit of the mask (t below the number of segments)
MDP_HD int we_last_col(uint32_t lastm, int t)
{
    for (int k = 0; k < t; k++) lastm &= lastm - 1u;
    return lastm ? __builtin_ctz(lastm) : -1;
}
// first(seg(c)): the highest first column at or below c
MDP_HD int we_first_col(uint32_t firstm, int c) { return 31 - __builtin_clz((firstm & (0xffffffffu >> (31 - c))) | 1u); }

// row(i): the record of row i, 0 <= i <= n; base(p): y[p], 0 <= p < n, asked for only with EMIT.  With EMIT, copies = the counted copies, cap =
// the counted edits, out_end = the end of the window's slice of the list (cap rows of WE_FIELDS below it are the window's).
template <bool EMIT, class Row, class Base>
MDP_HD WeCount we_walk(const Row &row, const Base &base, int n, const WsStruct &st, int end_id, uint64_t copies, int32_t cap, int32_t *out_end)
{
    WeCount k = { 0, 0, 0, 0, 0 };
    if (end_id == WE_START) return k;
    uint64_t passed = 0;                                        // landings on first(s) by sub or left the walk has behind it, 16 bits per segment
    int i = n, c = end_id < st.S ? we_last_col(st.last, end_id) : -1, have = -1, lefts = 0;
    WeRow rw = { 0, 0 };
    for (;;) {
        if (i < 0 || i > n || c < 0 || c >= st.W || lefts > 2 * st.W) { k.bad = 1; break; }
        if (have != i) { rw = row(i); have = i; }
        const int kind = (int)((rw.kinds >> (2 * c)) & 3u);
        const int s = (int)((st.seg >> (2 * c)) & 3u), sh = 16 * s;
        const bool isf = (st.first >> c) & 1u, isl = (st.last >> c) & 1u;
        if (kind != WE_LEFT && i < 1) { k.bad = 1; break; }      // row 0 has lefts only
        if (kind != WE_SUB) {
            if (EMIT) {
                if (k.edits >= cap) { k.bad = 1; break; }
                int32_t *o = out_end - (int64_t)WE_FIELDS * (k.edits + 1);
                o[0] = kind == WE_LEFT ? i : i - 1; o[1] = s;
                o[2] = (int)((copies >> sh) & 0xffffu) - (int)((passed >> sh) & 0xffffu) - 1;
                o[3] = c - we_first_col(st.first, c);
                o[4] = kind == WE_SUBX ? 0 : kind;
                o[5] = kind == WE_LEFT ? (int)((st.mot >> (2 * c)) & 3u) : (int)base(i - 1);
            }
            k.edits++;
        }
        if (kind == WE_UP) { i--; lefts = 0; continue; }
        const uint64_t one = (uint64_t)1 << sh;
        if (isl) k.copies += one;
        if (kind == WE_SUB) k.matches += one;
        const int di = kind == WE_LEFT ? 0 : 1;
        lefts = di ? 0 : lefts + 1;
        if (!isf) { c--; i -= di; continue; }
        passed += one;
        const int id = (int)((rw.ids >> (3 * s)) & 7u);
        if (id != s) k.entry = ws_set_entry<uint64_t>(k.entry, sh, i - di);
        if (id == WE_START) break;
        if (id > s) { k.bad = 1; break; }
        c = we_last_col(st.last, id); i -= di;
    }
    return k;
}
