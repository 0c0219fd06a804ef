// motif_dp.h — the wrap-around DP of ONE read against ONE short motif, forward pass and traceback, as one sequential function: the form the
// known-motif search runs one per lane (motif_search.hip.inc: 64 reads per wavefront, the motif wave-uniform).  Plain C++, nothing of HIP:
// the same functions compile into the gfx950 kernels and into a host program (tests/motif_dp_check.cpp).
//
// The definition is include/mtr_hip.h's ("known-motif search"): the reference's wrap_around_DP_sub (wrap_around_DP.c:222-354) with DP row i
// standing for read base x[i - 1].
//   forward     H(i, j) = diag + G on a match, else max(0, diag - MM, up - D, left - D), no left term in column 1; H(i, 0) = H(i, U).  The
//               previous row is an array of UB registers (UB = the bucket: 4, 8, 16, 32), the loop over the columns is unrolled over UB and cut
//               at U, so every index is a constant and U decides scalar branches.  The motif is 2 bits per base in a 64-bit value: on the GPU
//               a scalar register pair, base j a scalar bit-field extract.
//   best cell   the first strict maximum in row-major order: the loops ARE row-major, `>` is the whole rule.
//   cells       what the traceback needs of a cell are the four flags of mtr_common.h (H > 0, H != diag - MM, H != left - D, match), one byte
//               per cell, four columns per dword.  Column 1's "left" is the row's LAST column (wrap_around_DP.c:302, :314), known at the end of
//               the row: the row's first dword is stored last.  Where a dword goes is the Cells type's business: store(i, d, v) / load(i, d) for
//               row i (1-origin) and dword d of the row.  MdpCellsLane interleaves by lane - dword (i, d) of lane l at ((i - 1) * nd + d) * 64 + l
//               - so that one store instruction of a wavefront writes 256 contiguous bytes; a lane's slice is its own, whatever the other
//               lanes' lengths.
//   traceback   wrap_around_DP.c:298-333 on the flags: match, else stop at H == 0, else mismatch, deletion, insertion in that order.  One
//               dword load per (row, dword) visited.  A walk of more than (bi + 1) * (U + 1) steps cannot come from a consistent matrix:
//               score = -1 instead of spinning.
//   window      the locus search (motif_loci.hip.inc) aligns a WINDOW x[lo .. lo + L) of the read: the last argument `lo` of the forward pass
//               (default 0: the whole read) makes row i stand for base x[lo + i - 1], with the word and the phase of that position.  Nothing
//               else changes - the rows, the cells and every output are the window's own, as if its bases had been copied out.
#pragma once
#include "mtr_common.h"

#define MDP_HD static inline __host__ __device__ __attribute__((always_inline))
#define MDP_MEMBER inline __host__ __device__ __attribute__((always_inline))
#if defined(__clang__)
#define MDP_UNROLL _Pragma("unroll")
#else
#define MDP_UNROLL
#endif
#define MDP_MAX_U 32                      // the largest bucket: the motif's 2-bit codes fill a 64-bit value

struct MotifHit { int start, end, repeat_len, copies, mat, mis, ins, del, score; };    // the columns of include/mtr_hip.h, score last

MDP_HD int mdp_dwords(int U) { return (U + 3) >> 2; }                                     // dwords of cells per row
MDP_HD int mdp_bucket(int U) { return U <= 4 ? 4 : U <= 8 ? 8 : U <= 16 ? 16 : 32; }      // the UB a motif of U <= MDP_MAX_U bases runs with
// the motif's codes (0..3) as the 64-bit value the forward pass takes: base j at bits 2j
MDP_HD uint64_t mdp_motif_bits(const uint8_t *codes, int U)
{
    uint64_t m = 0;
    for (int j = 0; j < U && j < MDP_MAX_U; j++) m |= (uint64_t)(codes[j] & 3) << (2 * j);
    return m;
}

struct MdpCellsLane {
    uint32_t *p; int nd, lane;            // the wavefront's buffer (rows * nd * 64 dwords), dwords per row, this lane
    MDP_MEMBER void store(int i, int d, uint32_t v) const { p[((size_t)(i - 1) * (size_t)nd + (size_t)d) * 64 + (size_t)lane] = v; }
    MDP_MEMBER uint32_t load(int i, int d) const { return p[((size_t)(i - 1) * (size_t)nd + (size_t)d) * 64 + (size_t)lane]; }
};

// pk: the read in the device layout (2 bits per base, first base in the top bits of word 0); L >= 0 rows; 1 <= U <= UB; lo >= 0: the window's first base
template <int UB, class Cells>
MDP_HD void motif_dp_forward(const uint32_t *pk, int L, uint64_t mot, int U, int G, int MM, int D, const Cells &cells, int &best_v, int &best_i, int &best_j,
                             int lo = 0)
{
    static_assert(UB >= 1 && UB <= MDP_MAX_U, "bucket");
    int P[UB];
    MDP_UNROLL
    for (int j = 0; j < UB; j++) P[j] = 0;
    int wrap = 0, bv = 0, bi = 0, bj = 0;                    // wrap = H(i - 1, U)
    uint32_t w = 0;
    for (int i = 1; i <= L; i++) {
        const int p = lo + i - 1, b = p & 15;
        if (b == 0 || i == 1) w = pk[p >> 4];                   // (a window begins inside a word)
        const int xi = (int)((w >> (30 - 2 * b)) & 3u);
        int diag = wrap, left = 0;
        uint32_t acc = 0, first = 0;
    MDP_UNROLL
        for (int j = 0; j < UB; j++) {
            if (j < U) {
                const int mj = (int)((mot >> (2 * j)) & 3u);
                const int up = P[j];
                const bool m = xi == mj;
                const int t1 = diag - MM, t2 = up - D, t3 = left - D;
                int h = t1 > t2 ? t1 : t2;
                h = h > 0 ? h : 0;
                if (j > 0) h = h > t3 ? h : t3;
                const int H = m ? diag + G : h;
                uint32_t f = (H > 0 ? 1u : 0u) | (H != t1 ? 2u : 0u) | (m ? 8u : 0u);
                if (j > 0) f |= H != t3 ? 4u : 0u;             // (column 1: after the row)
                if (H > bv) { bv = H; bi = i; bj = j + 1; }
                acc |= f << (8 * (j & 3));
                if ((j & 3) == 3 || j == U - 1) {
                    if ((j >> 2) == 0) first = acc; else cells.store(i, j >> 2, acc);
                    acc = 0;
                }
                diag = up; P[j] = H; left = H;
            }
        }
        wrap = left;                                           // H(i, U)
        if (P[0] != wrap - D) first |= 4u;
        cells.store(i, 0, first);
    }
    best_v = bv; best_i = bi; best_j = bj;
}

template <class Cells>
MDP_HD MotifHit motif_dp_traceback(const Cells &cells, int U, int best_v, int best_i, int best_j)
{
    MotifHit r = { 0, -1, 0, 0, 0, 0, 0, 0, 0 };
    if (best_v <= 0) return r;
    int i = best_i, j = best_j, mat = 0, mis = 0, ins = 0, del = 0;
    long long guard = ((long long)best_i + 1) * ((long long)U + 1);
    int ci = 0, cd = 0; uint32_t w = 0;                          // the dword in hand: row ci (0 = none), dword cd
    while (i > 0) {
        const int d = (j - 1) >> 2;
        if (i != ci || d != cd) { w = cells.load(i, d); ci = i; cd = d; }
        const uint32_t f = (w >> (8 * ((j - 1) & 3))) & 15u;
        if (f & 8u) { mat++; i--; j--; }
        else if (!(f & 1u)) break;
        else if (!(f & 2u)) { mis++; i--; j--; }
        else if (!(f & 4u)) { del++; j--; }
        else { ins++; i--; }
        if (j == 0) j = U;
        if (--guard < 0) { r.score = -1; return r; }
    }
    r.start = i; r.end = best_i - 1; r.repeat_len = best_i - i; r.copies = (mat + mis + del) / U;
    r.mat = mat; r.mis = mis; r.ins = ins; r.del = del; r.score = best_v;
    return r;
}

// the two in a row: the single definition of a lane's work
template <int UB, class Cells>
MDP_HD MotifHit motif_dp(const uint32_t *pk, int L, uint64_t mot, int U, int G, int MM, int D, const Cells &cells, int lo = 0)
{
    int bv, bi, bj;
    motif_dp_forward<UB>(pk, L, mot, U, G, MM, D, cells, bv, bi, bj, lo);
    return motif_dp_traceback(cells, U, bv, bi, bj);
}
