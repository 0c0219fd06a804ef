// motif_loci.h — the rule of the known-motif LOCUS search (include/mtr_hip.h, "every locus of a motif"): what becomes of an aligned window of a
// read.  Plain C++, nothing of HIP: the same text compiles into the gfx950 kernels (motif_loci.hip.inc: mtr_k_loci_split, mtr_k_loci_bin) and into
// a host program (tests/motif_loci_check.cpp).
//
// The definition is a recursion over half-open windows x[lo .. hi) of a read, for a threshold S >= 1 and R rounds:
//   loci(lo, hi, depth):  hi - lo < minlen: nothing.  depth == R: the pair is "open", nothing more.  The window's hit (the known-motif search's, of
//   the window as a read of its own) scores below S: nothing.  Else the hit is a locus, and loci(lo, lo + start, depth + 1) and
//   loci(lo + end + 1, hi, depth + 1) follow, start and end being the hit's in window coordinates, end inclusive.
//   minlen = ceil(S / G): a window of fewer bases cannot score S, so leaving it out never changes a result.
// The kernels run the recursion level by level: round d aligns the windows of depth d, and mlo_split() says of each what round d + 1 gets.
#pragma once
#include "mtr_common.h"

#define MLO_HD static inline __host__ __device__ __attribute__((always_inline))
#define MLO_MAX_ROUNDS 32

MLO_HD int mlo_minlen(int S, int G) { return (S + G - 1) / G; }

// emit: the hit is a locus.  n: its children that go on (at most two, left first), windows clo[k] .. chi[k] of the read.  open: a child that
// would go on stands at depth R.
struct MloSplit { int emit, n, open, clo[2], chi[2]; };
// the window x[lo .. hi) aligned in round `depth` (0 <= depth < R); score, start, end: its hit in window coordinates (score 0: none)
MLO_HD MloSplit mlo_split(int lo, int hi, int depth, int R, int minlen, int S, int score, int start, int end)
{
    MloSplit s = { 0, 0, 0, { 0, 0 }, { 0, 0 } };
    if (score < S) return s;
    s.emit = 1;
    // (no array is indexed by a variable: on the GPU that would be a stack, and this runs one per lane)
    const int right = lo + end + 1;
    const bool l = start >= minlen, r = hi - right >= minlen, go = depth + 1 < R;
    s.open = !go && (l || r) ? 1 : 0;
    if (go && l) { s.clo[0] = lo; s.chi[0] = lo + start; s.n = 1; }
    if (go && r) {
        if (s.n == 0) { s.clo[0] = right; s.chi[0] = hi; } else { s.clo[1] = right; s.chi[1] = hi; }
        s.n++;
    }
    return s;
}

// The length class of a window of len >= 1 bases on the lane path: the windows of one wavefront are of one class, so that its 64 lanes end within
// a sixteenth of their rows of each other.  Lengths below 32 are classes of their own; from there on a class is the leading bit and the four bits
// behind it.  Monotone in len; below MLO_N_CLASSES for every len <= 16384 (MS_LANE_ROWS).
#define MLO_N_CLASSES 177
MLO_HD int mlo_len_class(int len)
{
    if (len < 32) return len;
    const int e = 31 - __builtin_clz((unsigned)len);          // 5 ..
    return 32 + (e - 5) * 16 + ((len >> (e - 4)) & 15);
}
