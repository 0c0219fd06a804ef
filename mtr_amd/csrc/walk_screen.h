// walk_screen.h — the nodes of a window and the dead-range screen of the staged unit search.  Plain C++, nothing of HIP: the same
// functions compile into the gfx950 kernels and into a host program (tests/walk_screen_check.cpp).
//
// A candidate range whose most frequent 2-mer node is seen at most MIN_NUM_FREQ_UNIT times yields nothing at k = 2
// (consensus.c:532), and the frequency bound of k2_range_walks gives it the cleared record at every larger k as well.  Learning
// that took a wavefront, a table in LDS and a handful of dependent round trips per range (mtr_k_walks); for a window of at most
// 64 bases it is 16 counters of at most 64, which one lane keeps in two registers (mtr_k_walk_screen, k3_staged.hip.inc).
#pragma once
#include "mtr_common.h"

#define MTR_HD static inline __host__ __device__ __attribute__((always_inline))

// ---- 2-bit packed reads: base i lives in word i>>4 at bit 30-2*(i&15) (MSB first) -----------------
// (PK: whatever yields word j as pk[j] - a pointer, or the window's words in registers, below)
template <class PK> MTR_HD int base_at(const PK &pk, int i) { return (int)(((uint32_t)pk[i >> 4] >> (30 - 2 * (i & 15))) & 3u); }
// value of the k-mer starting at i, first base most significant (consensus.c:46-57), k <= 15
template <class PK> MTR_HD int kmer_at(const PK &pk, int i, int k)
{
    unsigned long long x = ((unsigned long long)(uint32_t)pk[i >> 4] << 32) | (unsigned long long)(uint32_t)pk[(i >> 4) + 1];
    int sh = 64 - 2 * (i & 15) - 2 * k;
    return (int)((x >> sh) & ((1ull << (2 * k)) - 1ull));
}
// node of window position i: the k-mer at i while i < min(qe, L-k+1), else the raw base code
// (init_inputString, consensus.c:37-60)
template <class PK> MTR_HD int win_node(const PK &pk, int L, int k, int qe, int i)
{
    int lim = qe < L - k + 1 ? qe : L - k + 1;
    return i < lim ? kmer_at(pk, i, k) : base_at(pk, i);
}
// k range of a window (handle_one_read.c:106-118)
MTR_HD void k2_k_range(int w, int &min_k, int &max_k)
{
    if (w < 100) { min_k = MTRC_MIN_KMER - 3; max_k = MTRC_MAX_KMER - 5; }
    else if (w < 1000) { min_k = MTRC_MIN_KMER - 3; max_k = MTRC_MAX_KMER - 3; }
    else { min_k = MTRC_MIN_KMER; max_k = MTRC_MAX_KMER; }
}

// ---- the screen ------------------------------------------------------------------------------------------------------------------
#define WS_MAX_WIDTH 64                      // the widest window one lane counts: 16 counters of at most 64 in 8 bits each
#define WS_WORDS 5                           // 64 bases from any offset in a word span at most five words
// the packed words [w0, w0 + WS_WORDS) of a read, as many of them as the window [qs, qe] touches; any other word reads as zero (kmer_at
// always takes the word behind its own: behind the window's last word no node of the window has a base)
struct WsWords {
    uint32_t v[WS_WORDS]; int w0;
    inline __host__ __device__ __attribute__((always_inline)) uint32_t operator[](int j) const
    {   // (a chain of selects: indexing v[] by a variable would put the five words into scratch memory)
        const int d = j - w0;
        return d == 0 ? v[0] : d == 1 ? v[1] : d == 2 ? v[2] : d == 3 ? v[3] : d == 4 ? v[4] : 0u;
    }
};
MTR_HD void ws_load(WsWords &ww, const uint32_t *pk, int qs, int qe)
{
    ww.w0 = qs >> 4;
    const int n = (qe >> 4) - ww.w0 + 1;
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < WS_WORDS; q++) ww.v[q] = q < n ? pk[ww.w0 + q] : 0u;
}
// the rule covers windows that start at k = 2 (k2_k_range: w < 1000) and whose counters fit a lane
MTR_HD bool ws_applies(int qs, int qe, int w) { return w < 1000 && qe - qs + 1 <= WS_MAX_WIDTH; }
// the largest count among the 2-mer nodes of window [qs, qe] (ws_applies): what tab_build(k = 2) returns
template <class PK> MTR_HD int ws_max_freq(const PK &pk, int L, int qs, int qe)
{
    unsigned long long lo = 0ull, hi = 0ull;               // counters of nodes 0..7 and 8..15, a byte each
    for (int i = qs; i <= qe; i++) {
        const int node = win_node(pk, L, 2, qe, i);
        const unsigned long long one = 1ull << (8 * (node & 7));
        lo += node < 8 ? one : 0ull; hi += node < 8 ? 0ull : one;
    }
    // the maximum of the 16 bytes
    const unsigned long long m8 = 0x00ff00ff00ff00ffull;
    unsigned long long a = lo & m8, b = (lo >> 8) & m8, c = hi & m8, d = (hi >> 8) & m8;        // 4 x 4 counters in 16-bit fields
    unsigned mx = 0u;
    for (int q = 0; q < 4; q++) {
        const unsigned fa = (unsigned)(a >> (16 * q)) & 0xffffu, fb = (unsigned)(b >> (16 * q)) & 0xffffu;
        const unsigned fc = (unsigned)(c >> (16 * q)) & 0xffffu, fd = (unsigned)(d >> (16 * q)) & 0xffffu;
        const unsigned m1 = fa > fb ? fa : fb, m2 = fc > fd ? fc : fd, m3 = m1 > m2 ? m1 : m2;
        mx = m3 > mx ? m3 : mx;
    }
    return (int)mx;
}
// The range is dead - no candidate at k = 2, and every larger k skipped by the frequency bound - exactly when this holds: the test of
// search_walks for k = 2, then the test of k2_range_walks and of mtr_k_walks' `alive` loop for every larger k (a trailing raw-base node
// can add one to the bound each)
MTR_HD bool ws_dead(int max_freq, int L, int qe, int max_k)
{
    if (max_freq > MTRC_MIN_NUM_FREQ_UNIT) return false;
    for (int k = 3; k <= max_k; k++) {
        const int lim = qe < L - k + 1 ? qe : L - k + 1;
        if (max_freq + (qe - lim + 1) > MTRC_MIN_NUM_FREQ_UNIT) return false;
    }
    return true;
}
// one range: is it dead?  (pk = the read's packed words; the caller has tested ws_applies)
MTR_HD bool ws_range_dead(const uint32_t *pk, int L, int qs, int qe, int w, int *max_freq_out)
{
    WsWords ww; ws_load(ww, pk, qs, qe);
    const int mf = ws_max_freq(ww, L, qs, qe);
    if (max_freq_out) *max_freq_out = mf;
    int min_k, max_k;
    k2_k_range(w, min_k, max_k);
    return ws_dead(mf, L, qe, max_k);
}
