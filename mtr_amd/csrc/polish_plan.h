// polish_plan.h — polish_repeat (consensus.c:610-704) as a plan over the positions that matter.  Plain C++, nothing of HIP: the same
// functions compile into the gfx950 kernels (polish(), k2_units.hip.inc) and into a host program (tests/polish_plan_check.cpp).
//
// The reference walks the unit from its last base to its first.  At a position whose node frequency is 1 and which is suspicious (the
// flag predicate, pp_flagged) it looks five nodes up and may alter the unit; everywhere else it copies the base and goes one position down.
// Whether a position is flagged depends on the scores alone, so the flagged set is known before the walk starts (PpMask), and the walk
// becomes a sequence of events: copy a stretch, or run the reference's loop body at one position (pp_walk_plan).  The reference's loop
// itself is here too (pp_walk_all): the kernels run it under -DMTR_POLISH_WALK_ALL, and the host check holds the plan to it call for call.
//
// Both walks are written over an OPS object that says where things live (LDS and a wavefront on the GPU, arrays and a map on the host):
//   int  base(int j)                  base 0..3 of unit position j
//   int  score(int j)                 node frequency of position j, clamped to 0..3 (pp_clamp_score)
//   int  get(int node)                frequency of a node in the k-mer table of the repeat
//   void get4(a0, a1, a2, a3, int &f0, int &f1, int &f2, int &f3)     the same for four nodes at once (the GPU: a lane each)
//   int  cyc(int j)                   the unit's cyclic k-mer at j, 0 <= j < period (pp_cyc; the GPU answers it with one ballot)
//   void emit(int jr, int b)          out[jr] = b
//   void copy(int jr, int j, int n)   out[jr - i] = base(j - i) for 0 <= i < n
//   void undefined()                  the reference reads int_unit[-1] here: counted
//   void join()                       end of a loop body (device_util.hip.inc: loop_join)
#pragma once
#include "mtr_common.h"

#ifndef MTR_HD
#define MTR_HD static inline __host__ __device__ __attribute__((always_inline))
#endif

// ---- staging: one byte per position, bits 0-1 = base, bits 2-3 = min(max(score, 0), 3) (the walk only asks "== 1" and "< 2") ------------
MTR_HD int pp_clamp_score(int sv) { return sv < 0 ? 0 : (sv > 3 ? 3 : sv); }
MTR_HD unsigned char pp_stage_byte(int base, int sv) { return (unsigned char)((base & 3) | (pp_clamp_score(sv) << 2)); }

// ---- the flag predicate of one position: string_score[j] == 1 and suspicious (consensus.c:597-608, :629) -----------------------------------
// sc(t): the clamped score of position t.  The window of suspicious() is cut at the unit's start (0 <= j - i); the comparison is the
// reference's, in double.
template <class SC> MTR_HD bool pp_flagged(const SC &sc, int k, int j)
{
    if (sc(j) != 1) return false;
    int cnt = 0;
    for (int i = 0; i < k - 1 && 0 <= j - i; i++) if (sc(j - i) < 2) cnt++;
    return (double)(k - 1) * 0.8 < (double)cnt;
}

// ---- the flagged set: bit j of word j >> 6 ---------------------------------------------------------------------------------------------------
#define PP_MASK_WORDS 8
static_assert(MTRC_MAX_PERIOD <= 64 * PP_MASK_WORDS, "a unit's positions fit the mask");
// A mask type M answers word(q), 0 <= q < PP_MASK_WORDS.  PpMask keeps the words in an array (the host); the kernels keep word q in lane q
// (k2_units.hip.inc: PolMask - sixteen scalar registers held across the walk made mtr_k_polish spill scalars into vector registers).
struct PpMask {
    unsigned long long w[PP_MASK_WORDS];
    inline __host__ __device__ unsigned long long word(int q) const { return w[q]; }
};
template <class M> MTR_HD bool pp_mask_any(const M &m)
{
    unsigned long long any = 0ull;
    for (int q = 0; q < PP_MASK_WORDS; q++) any |= m.word(q);
    return any != 0ull;
}
template <class M> MTR_HD bool pp_mask_test(const M &m, int j) { return ((m.word(j >> 6) >> (j & 63)) & 1ull) != 0ull; }
// the next flagged position at or below j (0 <= j < 64 * PP_MASK_WORDS), -1 = none: a bit scan per word
template <class M> MTR_HD int pp_mask_next(const M &m, int j)
{
    unsigned long long w = m.word(j >> 6) & (~0ull >> (63 - (j & 63)));
    for (int q = j >> 6;; ) {
        if (w != 0ull) return q * 64 + 63 - __builtin_clzll(w);
        if (--q < 0) return -1;
        w = m.word(q);
    }
}
template <class SC> MTR_HD void pp_mask_build(PpMask &m, const SC &sc, int k, int period)
{   // the host's way; the GPU gives every lane its positions and makes the words by ballot (polish())
    for (int q = 0; q < PP_MASK_WORDS; q++) m.w[q] = 0ull;
    for (int j = 0; j < period; j++) if (pp_flagged(sc, k, j)) m.w[j >> 6] |= 1ull << (j & 63);
}

// ---- what both walks share -------------------------------------------------------------------------------------------------------------------
// the unit's cyclic k-mer at j: bases j, j + 1, .. j + k - 1 (mod period), first base most significant
template <class OPS> MTR_HD int pp_cyc(OPS &ops, int k, int period, int j)
{
    int node = 0;
    for (int i = 0; i < k; i++) node = node * 4 + ops.base((j + i) % period);
    return node;
}
// score_for_alignment, consensus.c:584-595
template <class OPS> MTR_HD int pp_align_score(OPS &ops, int start, int k, int node, int period)
{
    int sum = 0;
    const int p4k1 = 1 << (2 * (k - 1));
    for (int j = start; 0 <= j && start - k < j; j--) { node = ops.base(j % period) * p4k1 + node / 4; sum += ops.get(node); }
    return sum;
}
// The reference's loop body at position j (consensus.c:623-644).  node: in, the node the walk arrived with; out, the node it leaves with.
// Returns whether the position was altered (the node it leaves with is not the unit's own, `ref`).
template <class OPS> MTR_HD bool pp_body(OPS &ops, int k, int period, int j, bool flagged, int &node, int &emit, int &step)
{
    const int p4k1 = 1 << (2 * (k - 1)), p4k = 1 << (2 * k);
    const int uj = ops.base(j);
    const int ref = uj * p4k1 + node / 4;
    node = ref;
    emit = uj; step = 1;
    if (!flagged) return false;
    // (only a flagged position looks nodes up.)  The four nodes that differ from ref in the first base alone: alt_l has base l there, so
    // alt_uj IS ref - the reference's fifth look-up, tab_get(ref), is f of alt_uj.  Every alt_l lies in [0, 4^k): its `% 4^k` (:628) is the
    // mask.  One get4, so that a wavefront can ask for the four side by side; then the reference's rule, the first maximum above ref's.
    const int a0 = (ref + (0 - uj) * p4k1) & (p4k - 1), a1 = (ref + (1 - uj) * p4k1) & (p4k - 1);
    const int a2 = (ref + (2 - uj) * p4k1) & (p4k - 1), a3 = (ref + (3 - uj) * p4k1) & (p4k - 1);
    int f0, f1, f2, f3;
    ops.get4(a0, a1, a2, a3, f0, f1, f2, f3);
    int bestf = uj == 0 ? f0 : uj == 1 ? f1 : uj == 2 ? f2 : f3;
    if (bestf < f0) { bestf = f0; node = a0; }
    if (bestf < f1) { bestf = f1; node = a1; }
    if (bestf < f2) { bestf = f2; node = a2; }
    if (bestf < f3) { bestf = f3; node = a3; }
    if (node == ref) return false;
    const int sd = pp_align_score(ops, j, k, node, period);
    const int ss = pp_align_score(ops, j - 1, k, node, period);
    int si = -1;
    int prevb;
    if (j == 0) { prevb = -1; ops.undefined(); }               // int_unit[-1] in the reference (H10)
    else prevb = ops.base((j - 1) % period);
    if (node / p4k1 == prevb) si = pp_align_score(ops, j - 2, k, node, period);
    emit = node / p4k1;
    int mx = sd > ss ? sd : ss; if (si > mx) mx = si;
    step = (mx == sd) ? 0 : (mx == ss ? 1 : 2);
    return true;
}

// ---- the reference's walk: every position, last to first ------------------------------------------------------------------------------------
// Emits into out[jr], jr = MTRC_MAX_PERIOD - 1 downwards.  false: the output outgrew MTRC_MAX_PERIOD and the unit stays as it was (:645);
// else the polished unit is out[jr + 1 .. MTRC_MAX_PERIOD - 1].  altered: some position left with another node than the unit's own -
// without one the output is the input.
template <class OPS> MTR_HD bool pp_walk_all(OPS &ops, int k, int period, int &jr_out, bool &altered)
{
    int jr = MTRC_MAX_PERIOD - 1;
    int node = 0;
    for (int i = 0; i < k; i++) node += ops.base(i) * (1 << (2 * (k - 1 - i)));
    bool ok = true;
    altered = false;
    for (int j = period - 1; 0 <= j;) {
        int emit, step;
        const bool fl = pp_flagged([&](int t) { return ops.score(t); }, k, j);
        if (pp_body(ops, k, period, j, fl, node, emit, step)) altered = true;
        ops.emit(jr, emit);
        jr--; j -= step;
        ops.join();
        if (jr < 0) { ok = false; break; }
    }
    jr_out = jr;
    return ok;
}

// ---- the plan: the same walk as a sequence of events ------------------------------------------------------------------------------------------
// State: (j, jr, node, clean).  clean = the node the walk arrives at j with is the unit's own, cyc(j + 1): what the loop's `ref` recurrence
// gives when nothing above j has been altered (at the start: cyc(0), the reference's first node, and j + 1 = period wraps to 0).
//   clean, and j above the next flagged position f: a clean, unflagged position can only take the `else { emit = uj; step = 1; }` arm, and
//     that arm leaves node == ref, the unit's own k-mer of that position - so the next position is reached clean as well, and the whole
//     stretch j .. f + 1 is a copy of the unit's bases.  The output's overflow (:645) is checked for the stretch as a whole: n emissions
//     from jr leave jr - n, negative exactly when n > jr.
//   at a flagged position, or whenever not clean: the reference's loop body (pp_body).  Arriving clean, the node is cyc(j + 1).
//   after a body step that altered the unit, or one taken while not clean, the state is clean again only if the node IS the cyclic k-mer
//     the next position expects - compared, not counted: steps of 0 and 2 move j against the node's digits.
template <class OPS, class M> MTR_HD bool pp_walk_plan(OPS &ops, const M &m, int k, int period, int &jr_out, bool &altered)
{
    int jr = MTRC_MAX_PERIOD - 1;
    int node = ops.cyc(0);                                     // the reference's first node (:621; period > k: no wrap in it)
    bool ok = true, clean = true;
    altered = false;
    for (int j = period - 1; 0 <= j;) {
        if (clean) {
            const int f = pp_mask_next(m, j);
            const int n = j - f;                               // the unflagged positions j .. f + 1
            if (n > 0) {
                if (n > jr) { ok = false; break; }
                ops.copy(jr, j, n);
                jr -= n; j = f;
                if (j < 0) break;
                node = ops.cyc(j + 1);                         // (behind a stretch j + 1 < period; without one the node is the last step's)
            }
        }
        int emit, step;
        const bool alt = pp_body(ops, k, period, j, pp_mask_test(m, j), node, emit, step);
        if (alt) altered = true;
        ops.emit(jr, emit);
        jr--; j -= step;
        ops.join();
        if (jr < 0) { ok = false; break; }
        if (alt || !clean) clean = 0 <= j && node == ops.cyc(j + 1 == period ? 0 : j + 1);
    }
    jr_out = jr;
    return ok;
}
