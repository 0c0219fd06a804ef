// banded_align.h — the allele consensus' banded global alignment of ONE member window W[0 .. n) to its backbone B[0 .. m): the band, the cell
// with its direction rule, the anti-diagonal schedule one wavefront runs (consensus.hip.inc: mtr_k_cons_align), the traceback that votes, and
// the emission of one backbone position.  Plain C++, nothing of HIP: the same functions compile into the gfx950 kernels and into a host program
// (tests/banded_align_check.cpp), which holds them to a brute-force full matrix.
//
// The definition is include/mtr_hip.h's ("allele consensus"):
//   band        cells (i, j), 0 <= i <= n, 0 <= j <= m, exist iff dlo <= j - i <= dhi, dlo = min(0, m - n) - band_extra, dhi = max(0, m - n) +
//               band_extra; every other cell is infinite
//   D           D(0, 0) = 0, else the minimum of diag = D(i-1, j-1) + (W[i-1] != B[j-1]), up = D(i-1, j) + 1, left = D(i, j-1) + 1; the cell's
//               direction is the FIRST of diag, up, left that attains the minimum
//   votes       from (n, m) to (0, 0) by the directions: diag -> base[j][W[i-1]], left -> del[j], a maximal run of up steps at column j -> its
//               first BA_INS_SLOTS bases in read order into ins[j][k][.]
// The schedule: on anti-diagonal s = i + j only the diagonals d = j - i of s' parity hold a cell, and a cell's three inputs lie on the two
// anti-diagonals before it.  Band diagonal e = d - dlo; the diagonals 2p and 2p + 1 are PAIR p, whose two running values are (E, O).  With
// par = (s - dlo) & 1 the step computes, for every pair, e = 2p + par:
//   par = 0     E' = cell(diag = E (of s - 2), up = O (of s - 1), left = O of pair p - 1)
//   par = 1     O' = cell(diag = O,            up = E of pair p + 1,                left = E)
// so a step needs ONE neighbour value, alternately from below and from above.  A cell outside the matrix or the band is stored as BA_INF; with
// that no border needs a case of its own except (0, 0).  The directions go, 2 bits each, 16 steps a dword, to word ba_dir_word(s, p, cpl).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_HD static inline __host__ __device__ __attribute__((always_inline))
#else
#define BA_HD static inline __attribute__((always_inline))
#endif

#define BA_MAX_WINDOW 16384        // MTR_CONS_MAX_WINDOW
#define BA_MAX_BAND 256            // MTR_CONS_MAX_BAND
#define BA_INS_SLOTS 4             // MTR_CONS_INS_SLOTS
#define BA_MAX_EXTRA 64
#define BA_TAB (4 + 1 + 4 * BA_INS_SLOTS)   // int32 per backbone position 0 .. m: base[4], del, ins[slot][4]
#define BA_TAB_DEL 4
#define BA_TAB_INS 5
#define BA_INF (1 << 29)
#define BA_DIAG 0
#define BA_UP 1
#define BA_LEFT 2

struct BaBand { int32_t dlo, dhi; };

BA_HD BaBand ba_band(int32_t n, int32_t m, int32_t extra)
{
    BaBand b;
    b.dlo = (m - n < 0 ? m - n : 0) - extra; b.dhi = (m - n > 0 ? m - n : 0) + extra;
    return b;
}
BA_HD int32_t ba_width(const BaBand &b) { return b.dhi - b.dlo + 1; }

// is the member of n bases left out of the backbone's (m bases) vote?
BA_HD bool ba_skipped(int64_t n, int64_t m, int32_t extra)
{
    const int64_t diff = m > n ? m - n : n - m;
    return n > BA_MAX_WINDOW || m > BA_MAX_WINDOW || diff + 2 * (int64_t)extra + 1 > BA_MAX_BAND;
}

// one cell from its three inputs (BA_INF: none), each before its own cost is added
BA_HD int32_t ba_cell(int32_t diag, int32_t up, int32_t left, bool mismatch, int &dir)
{
    int32_t best = diag + (mismatch ? 1 : 0);
    dir = BA_DIAG;
    if (up + 1 < best) { best = up + 1; dir = BA_UP; }
    if (left + 1 < best) { best = left + 1; dir = BA_LEFT; }
    return best < BA_INF ? best : BA_INF;
}

// the cell of band diagonal e on anti-diagonal s ((s - dlo - e) even), from the running values named above
BA_HD int32_t ba_step_cell(int32_t s, int32_t e, int32_t n, int32_t m, const BaBand &b, int32_t diag, int32_t up, int32_t left, const uint8_t *W,
                           const uint8_t *B, int &dir)
{
    const int32_t d = b.dlo + e, i2 = s - d, j2 = s + d;
    dir = BA_DIAG;
    if (d > b.dhi || i2 < 0 || j2 < 0 || i2 > 2 * n || j2 > 2 * m) return BA_INF;
    if (s == 0) return 0;
    const int32_t i = i2 >> 1, j = j2 >> 1;
    const bool mismatch = i >= 1 && j >= 1 ? W[i - 1] != B[j - 1] : true;       // (without a diagonal input the cost does not matter)
    return ba_cell(diag, up, left, mismatch, dir);
}

// where pair p's directions of anti-diagonal s lie: lane p / cpl holds the pairs p - p % cpl .. of which this is number p % cpl
BA_HD int64_t ba_dir_word(int32_t s, int32_t p, int32_t cpl) { return ((int64_t)(s >> 4) * cpl + p % cpl) * 64 + p / cpl; }
BA_HD int64_t ba_dir_words(int32_t n, int32_t m, int32_t cpl) { return ((int64_t)((n + m) >> 4) + 1) * cpl * 64; }
BA_HD int ba_dir_at(const uint32_t *dirs, int32_t i, int32_t j, int32_t dlo, int32_t cpl)
{
    const int32_t s = i + j, p = (j - i - dlo) >> 1;
    return (int)((dirs[ba_dir_word(s, p, cpl)] >> (2 * (s & 15))) & 3u);
}

// the whole fill in the kernel's schedule by ONE thread: E, O hold 64 * cpl values each, dirs ba_dir_words(n, m, cpl) words; the band is at most
// 128 * cpl diagonals wide.  Returns D(n, m).
// The kernel runs the same steps with pair p in lane p / cpl; this is what the host check and the host timing run.
BA_HD int32_t ba_fill(int32_t n, int32_t m, const uint8_t *W, const uint8_t *B, const BaBand &b, int32_t cpl, int32_t *E, int32_t *O, uint32_t *dirs)
{
    const int32_t pairs = (ba_width(b) + 1) >> 1;                              // (<= 64 * cpl; the pairs behind the band stay BA_INF in the kernel)
    for (int64_t w = 0, nw = ba_dir_words(n, m, cpl); w < nw; w++) dirs[w] = 0u;
    for (int32_t p = 0; p < pairs; p++) E[p] = O[p] = BA_INF;
    for (int32_t s = 0; s <= n + m; s++) {
        const int par = (s - b.dlo) & 1;
        for (int32_t p = par ? 0 : pairs - 1; p >= 0 && p < pairs; p += par ? 1 : -1) {     // (in an order that reads the neighbour before it could change: it does not change in this step anyway)
            int dir;
            if (par == 0) E[p] = ba_step_cell(s, 2 * p, n, m, b, E[p], O[p], p > 0 ? O[p - 1] : BA_INF, W, B, dir);
            else O[p] = ba_step_cell(s, 2 * p + 1, n, m, b, O[p], p + 1 < pairs ? E[p + 1] : BA_INF, E[p], W, B, dir);
            dirs[ba_dir_word(s, p, cpl)] |= (uint32_t)dir << (2 * (s & 15));
        }
    }
    const int32_t e = m - n - b.dlo;
    return (e & 1) ? O[e >> 1] : E[e >> 1];
}

// the walk from (n, m) to (0, 0): dir_at(i, j) gives a cell's direction, vote(x) adds 1 to counter x of the backbone's table
// (position j's counters are x = j * BA_TAB ..).  Row 0 can only go left and column 0 only up, whatever dir_at says: the walk ends.
template <class DirAt, class Vote>
BA_HD void ba_walk(int32_t n, int32_t m, const uint8_t *W, DirAt dir_at, Vote vote)
{
    int32_t i = n, j = m;
    while (i > 0 || j > 0) {
        const int d = i == 0 ? BA_LEFT : j == 0 ? BA_UP : dir_at(i, j);
        if (d == BA_DIAG) { vote((int64_t)j * BA_TAB + W[i - 1]); i--; j--; }
        else if (d == BA_UP) {
            const int32_t end = i;                                              // the run is W[i .. end) once i has come down
            i--;
            while (i > 0 && (j == 0 || dir_at(i, j) == BA_UP)) i--;
            for (int32_t k = 0; k < BA_INS_SLOTS && i + k < end; k++) vote((int64_t)j * BA_TAB + BA_TAB_INS + 4 * k + W[i + k]);
        }
        else { vote((int64_t)j * BA_TAB + BA_TAB_DEL); j--; }
    }
}

// what backbone position j (0 .. m) emits: t = its BA_TAB counters (the aligned members' votes), bb = B[j - 1] (any value for j = 0), N = 1 + the
// aligned members.  The backbone's own vote is added here.  sym / votes [1 + BA_INS_SLOTS]: entry 0 is the position's base (emitted iff the
// result's bit 0 is set), entry 1 + k insertion slot k; returns has_base | n_ins << 1: the symbols are entry 0, if emitted, then entries 1 .. n_ins.
BA_HD int ba_emit(const int32_t *t, int32_t j, int bb, int32_t N, uint8_t *sym, int32_t *votes)
{
    int has_base = 0, n_ins = 0;
    sym[0] = 0; votes[0] = 0;
    if (j >= 1) {
        int best = 0; int32_t bv = -1;
        for (int c = 0; c < 4; c++) { const int32_t v = t[c] + (c == bb ? 1 : 0); if (v > bv) { bv = v; best = c; } }
        if (t[bb] + 1 == bv) best = bb;                                         // a tie goes to the backbone's base
        if (!(t[BA_TAB_DEL] > bv)) { sym[0] = (uint8_t)best; votes[0] = bv; has_base = 1; }
    }
    bool open = true;
    for (int k = 0; k < BA_INS_SLOTS; k++) {
        const int32_t *ins = t + BA_TAB_INS + 4 * k;
        int best = 0; int32_t mx = -1, tot = 0;
        for (int c = 0; c < 4; c++) { tot += ins[c]; if (ins[c] > mx) { mx = ins[c]; best = c; } }
        open = open && mx > N - tot;                                            // the first slot not emitted ends the junction
        sym[1 + k] = (uint8_t)best; votes[1 + k] = mx;
        n_ins += open ? 1 : 0;
    }
    return has_base | (n_ins << 1);
}

// ---- the quality-weighted vote (include/mtr_hip.h, "quality-weighted allele consensus") --------------------------------------------------------
// The alignment is the one above - band, D, directions, schedule -; only what a step of the walk adds to the table changes, and the table gets
// one more kind of counter: end[L], the boundary weight of a member whose insertion run behind the position has exactly L < BA_INS_SLOTS bases.
#define BAQ_MAX_CAP 93             // MTR_CONSQ_MAX_CAP
#define BAQ_TAB (BA_TAB + BA_INS_SLOTS)     // int32 per backbone position 0 .. m: base[4], del, ins[slot][4], end[4]
#define BAQ_TAB_END (BA_TAB_INS + 4 * BA_INS_SLOTS)

// the weight of a base of quality q
BA_HD int32_t baq_weight(int32_t q, int32_t cap) { return q < 1 ? 1 : q > cap ? cap : q; }
// the gap weight at boundary i (0 .. n) of a window of n bases whose qualities are Q: the lighter of the two bases beside it, the one that exists
// at the ends, 1 for an empty window
BA_HD int32_t baq_gap(const uint8_t *Q, int32_t n, int32_t i, int32_t cap)
{
    if (n == 0) return 1;
    const int32_t a = baq_weight(Q[i > 0 ? i - 1 : 0], cap), b = baq_weight(Q[i < n ? i : n - 1], cap);
    return a < b ? a : b;
}

// the walk from (n, m) to (0, 0), column by column: in column j the path's rows are lo .. hi, its run of up steps inserts W[lo .. hi) behind
// backbone position j, and it leaves column j >= 1 from (lo, j) by diag or left.  dir_at as for ba_walk; vote(x, w) adds w to counter x of the
// backbone's table (position j's counters are x = j * BAQ_TAB ..).  Q: the qualities of W.
template <class DirAt, class Vote>
BA_HD void baq_walk(int32_t n, int32_t m, const uint8_t *W, const uint8_t *Q, int32_t cap, DirAt dir_at, Vote vote)
{
    int32_t i = n;
    for (int32_t j = m; j >= 0; j--) {
        const int32_t hi = i;
        int d = BA_LEFT;                                                        // of (lo, j) once the run has ended above row 0
        while (i > 0) { d = j == 0 ? BA_UP : dir_at(i, j); if (d != BA_UP) break; i--; }
        const int64_t at = (int64_t)j * BAQ_TAB;
        for (int32_t k = 0; k < BA_INS_SLOTS && i + k < hi; k++) vote(at + BA_TAB_INS + 4 * k + W[i + k], baq_weight(Q[i + k], cap));
        if (hi - i < BA_INS_SLOTS) vote(at + BAQ_TAB_END + (hi - i), baq_gap(Q, n, hi, cap));
        if (j == 0) break;
        if (i > 0 && d == BA_DIAG) { vote(at + W[i - 1], baq_weight(Q[i - 1], cap)); i--; }
        else vote(at + BA_TAB_DEL, baq_gap(Q, n, i, cap));
    }
}

// what backbone position j (0 .. m) emits: t = its BAQ_TAB counters (the aligned members' weights), bb = B[j - 1] and wbb = its weight (any
// values for j = 0), gap = the backbone's own gap weight at boundary j.  The backbone's votes are added here.  sym / votes and the result as
// for ba_emit; votes are weight sums.
BA_HD int baq_emit(const int32_t *t, int32_t j, int bb, int32_t wbb, int32_t gap, uint8_t *sym, int32_t *votes)
{
    int has_base = 0, n_ins = 0;
    sym[0] = 0; votes[0] = 0;
    if (j >= 1) {
        int best = 0; int32_t bv = -1;
        for (int c = 0; c < 4; c++) { const int32_t v = t[c] + (c == bb ? wbb : 0); if (v > bv) { bv = v; best = c; } }
        if (t[bb] + wbb == bv) best = bb;                                       // a tie goes to the backbone's base
        if (!(t[BA_TAB_DEL] > bv)) { sym[0] = (uint8_t)best; votes[0] = bv; has_base = 1; }
    }
    bool open = true;
    int32_t none = gap;
    for (int k = 0; k < BA_INS_SLOTS; k++) {
        const int32_t *ins = t + BA_TAB_INS + 4 * k;
        int best = 0; int32_t mx = -1;
        for (int c = 0; c < 4; c++) if (ins[c] > mx) { mx = ins[c]; best = c; }
        none += t[BAQ_TAB_END + k];
        open = open && mx > none;                                               // the first slot not emitted ends the junction
        sym[1 + k] = (uint8_t)best; votes[1 + k] = mx;
        n_ins += open ? 1 : 0;
    }
    return has_base | (n_ins << 1);
}
