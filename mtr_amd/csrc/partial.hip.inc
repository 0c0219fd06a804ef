// partial.hip.inc — partial genotype (mtr_genotype_partial_device): what a read says of a locus (left flank, motif, right flank) that it does NOT
// span - one flank found, and the repeat running from it towards the read's end.  The flank step is the genotype's (flank_search.hip.inc's launches
// over four slots per locus: A, B, rc A, rc B).  What is new here:
//   mtr_k_partial_pair   one lane per (read, locus): the genotype's pairing rule exactly as mtr_k_geno_pair evaluates it - a row it would call
//                        spanning is none of ours - then the slot of smallest distance within K (the lowest slot on a tie), which fixes the
//                        window, the direction and the motif's VARIANT (4 * locus + M, reversed M, rc M, reversed rc M: the 64-bit values are the
//                        host's).  A partial row with a non-empty window appends one task (row, lo, hi, variant) to its variant's list - a variant
//                        belongs to one locus, so a list holds at most n_reads tasks - and remembers the place it drew: the order of the appends
//                        reaches no result.
//   mtr_k_ext_lanes<UB>  the hot path: ONE ANCHORED EXTENSION PER LANE (motif_ext.h, the single definition), 64 consecutive tasks of one variant
//                        per wavefront, so the motif is wave-uniform (two scalar registers).  The previous row of H, C and T is 3 * UB registers
//                        per lane; nothing is stored per cell: no scratch, no LDS, no traceback.  A wavefront is one GROUP of the work list the
//                        host made from the lists' counts (entries (variant, first group), the entry found by bisection on wave-uniform values,
//                        as the search's); a bucket's variants are one launch.  No cross-lane operation after the group is found.
//   mtr_k_partial_out    one lane per (read, locus): the caller's columns.
// partial_choose, partial_variant, partial_row_store and partial_row_out are the pairing's and the output's single definitions: the call at
// catalogue scale (partial_catalog.hip.inc) runs them per candidate.
#pragma once
#include "flank_search.hip.inc"
#include "motif_search.hip.inc"
#include "motif_ext.h"

#define PT_SLOTS 4                  // flank slots per locus: A, B, rc A, rc B (the genotype's)
#define PT_ROW 8                    // int32 per (read, locus): partial, slot, the slot's distance, lo, hi, the task's place in its list (-1: none), two spare
#define PT_EXT 4                    // int32 per (read, locus) with a task: MotifExt

struct PtTask { int32_t row, lo, hi, variant; };

struct PartialPairArgs {
    const int32_t *flank;           // [read * PT_SLOTS * n_loci + PT_SLOTS * locus + slot][FL_RES]
    const int32_t *lens;
    int32_t n_loci, K, n_reads; int64_t rows;
    int32_t *row;                   // [rows][PT_ROW]
    PtTask *tasks;                  // [variant][n_reads]
    int32_t *count;                 // [variant]
    int32_t *status;
};

// what the pairing makes of the four entries f = [slot][FL_RES] of one (read, locus) of a read of L bases: slot < 0 - spanning by the genotype's
// rule, or no slot within K - or the chosen slot, its distance and its window.  The one definition: the catalogue call's pairing runs it too.
struct PtChoice { int slot, dist, lo, hi; };
DEVINL PtChoice partial_choose(const int32_t *f, int K, int L, int32_t *status)
{
    const int32_t *A = f, *B = f + FL_RES, *rA = f + 2 * FL_RES, *rB = f + 3 * FL_RES;
    const bool v0 = A[0] <= K && B[0] <= K && A[2] <= B[1];
    const bool v1 = rA[0] <= K && rB[0] <= K && rB[2] <= rA[1];
    PtChoice c = { -1, 0, 0, 0 };
    if (!(v0 || v1)) {
        for (int s = 0; s < PT_SLOTS; s++) {
            const int d = f[s * FL_RES];
            if (d <= K && (c.slot < 0 || d < c.dist)) { c.slot = s; c.dist = d; }
        }
    }
    if (c.slot >= 0) {
        const int32_t *h = f + c.slot * FL_RES;
        if (c.slot == 0 || c.slot == 3) { c.lo = h[2]; c.hi = L; } else { c.lo = 0; c.hi = h[1]; }
        if (c.lo < 0 || c.hi > L || c.lo > c.hi) { atomicCAS(status, 0, DEV_ERR_INTERNAL); c.hi = c.lo = 0; }      // (a flank hit lies inside its read)
    }
    return c;
}
DEVINL int partial_variant(int l, int slot) { return 4 * l + (slot == 2 ? 3 : slot == 3 ? 2 : slot); }
// q: the PT_ROW values of a (read, locus); at: its task's place in its list, -1 without one
DEVINL void partial_row_store(int32_t *q, const PtChoice &c, int at)
{
    q[0] = c.slot >= 0 ? 1 : 0; q[1] = c.slot >= 0 ? c.slot : 0; q[2] = c.dist; q[3] = c.lo; q[4] = c.hi; q[5] = at; q[6] = 0; q[7] = 0;
}

__global__ __launch_bounds__(256) void mtr_k_partial_pair(PartialPairArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.rows) return;
    const int rd = (int)(p / a.n_loci), l = (int)(p - (int64_t)rd * a.n_loci);
    const PtChoice c = partial_choose(a.flank + (size_t)p * PT_SLOTS * FL_RES, a.K, a.lens[rd], a.status);
    int at = -1;
    if (c.slot >= 0 && c.hi > c.lo) {
        const int variant = partial_variant(l, c.slot);
        at = atomicAdd(&a.count[variant], 1);
        if (at >= a.n_reads) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); at = -1; }
        else a.tasks[(size_t)variant * (size_t)a.n_reads + (size_t)at] = { (int32_t)p, c.lo, c.hi, variant };
    }
    partial_row_store(a.row + (size_t)p * PT_ROW, c, at);
}

struct PartialExtArgs {
    BatchView b;
    const PtTask *tasks; const int32_t *count;          // per variant: its list of n_reads places, the tasks it holds
    const uint64_t *bits; const int32_t *ulen;          // per variant: the motif as motif_ext takes it; per locus: its length
    int32_t n_reads, n_loci, G, MM, D;
    MsWork work;                                        // entries (variant, first group); items = groups of 64 tasks
    int32_t *ext;                                       // [row][PT_EXT]
    int32_t *status;
};

template <int UB>
__global__ __launch_bounds__(64) void mtr_k_ext_lanes(PartialExtArgs a)
{
    const long long g = (long long)blockIdx.x;
    if (g >= a.work.n_items) return;
    const int e = ms_entry(a.work, g);
    const int v = uni(a.work.slot[e]);
    const int U = uni(a.ulen[v >> 2]);
    const uint64_t mot = (uint64_t)uni64((long long)a.bits[v]);
    const long long k = (g - uni64(a.work.first[e])) * 64 + lane_id();      // this lane's task of the variant's list
    PtTask t = { 0, 0, 0, v };
    const uint32_t *pk = a.b.packed;
    if (k < (long long)uni(a.count[v])) {
        t = a.tasks[(size_t)v * (size_t)a.n_reads + (size_t)k];
        const int rd = t.row / a.n_loci;
        pk = a.b.packed + a.b.woff[rd];
        if (t.lo < 0 || t.hi > a.b.lens[rd] || t.lo >= t.hi || U < 1 || U > UB) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); t.lo = t.hi = 0; }
    }
    if (t.hi <= t.lo) return;
    const FbvLoadGlobal ld = { pk };
    const MotifExt r = motif_ext<UB>(ld, t.lo, t.hi, v & 1, mot, U, a.G, a.MM, a.D);
    int32_t *o = a.ext + (size_t)t.row * PT_EXT;
    o[0] = r.ext_len; o[1] = r.motif_bases; o[2] = r.matches; o[3] = r.score;
}

struct PartialOut { uint8_t *partial, *slot; int32_t *flank_dist, *window, *ext; float *ratio; uint8_t *open; };
// one row's columns at place p: q = its PT_ROW values, x = its PT_EXT values (read only where the row has a task), U = its locus' motif length.
// The one definition of copies, tail, ratio and open: the catalogue call's output kernel runs it too.
DEVINL void partial_row_out(const int32_t *q, const int32_t *x, int U, int max_tail, int64_t p, const PartialOut &out)
{
    out.partial[p] = (uint8_t)q[0]; out.slot[p] = (uint8_t)q[1];
    out.flank_dist[p] = q[2];
    out.window[2 * p] = q[3]; out.window[2 * p + 1] = q[4];
    int32_t *o = out.ext + (size_t)p * 6;
    const int n = q[4] - q[3];
    int len = 0, C = 0, T = 0, H = 0;
    if (q[5] >= 0) { len = x[0]; C = x[1]; T = x[2]; H = x[3]; }
    o[0] = len; o[1] = C; o[2] = C / U; o[3] = T; o[4] = H; o[5] = n - len;
    out.ratio[p] = len > 0 ? (float)T / (float)len : 0.0f;
    out.open[p] = (uint8_t)(q[0] && n - len <= max_tail ? 1 : 0);
}

// ext: the tasks' results by row; a row without a task - not partial, or an empty window - has zeros
__global__ __launch_bounds__(256) void mtr_k_partial_out(const int32_t *row, const int32_t *ext, const int32_t *ulen, int32_t n_loci, int32_t max_tail, int64_t rows,
                                                         PartialOut out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows) return;
    partial_row_out(row + (size_t)p * PT_ROW, ext + (size_t)p * PT_EXT, ulen[(int)(p % n_loci)], max_tail, p, out);
}
