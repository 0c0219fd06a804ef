// genotype.hip.inc — locus genotyping (mtr_genotype_loci_device): a locus is (left flank, motif, right flank); a read spans it where both flanks
// are found in order, and the repeat between them is aligned to the motif.  The flank step is flank_search.hip.inc's launches over four slots per
// locus (A, B, rc A, rc B); the alignment step is ONE round of the locus search's path (motif_loci.hip.inc: mtr_k_loci_bin .. mtr_k_motif_loci_lanes<UB>,
// mtr_k_motif_loci_waves, unchanged), to which the genotype presents 2 * n_loci single-strand "motifs" - locus l in orientation o is motif
// 2 * l + o, the motif as given or its reverse complement - so that pair = read * (2 * n_loci) + 2 * l + o and task = interval.  What is new here:
//   mtr_k_geno_pair   one lane per (read, locus): include/mtr_hip.h's pairing rules on the four flank hits - the valid orientations, the smaller sum of
//                     distances, orientation 0 on a tie - then one interval appended per spanning pair with a non-empty window.  The order of the
//                     appends reaches no result: the pair remembers its interval's index.
//   mtr_k_geno_out    one lane per (read, locus): the caller's columns - the pairing's values, and the interval's hit moved to read coordinates.
#pragma once
#include "flank_search.hip.inc"
#include "motif_loci.hip.inc"

#define GT_SLOTS 4                  // flank slots per locus: A, B, rc A, rc B
#define GT_PAIR 8                   // int32 per (read, locus): spanning, orientation, left and right distance, lo, hi, the interval (-1: none), a spare

struct GenoPairArgs {
    const int32_t *flank;           // [read * GT_SLOTS * n_loci + GT_SLOTS * locus + slot][FL_RES]
    int32_t n_loci, K; int64_t rows;
    int32_t *pair;                  // [rows][GT_PAIR]
    LociIv *iv; int32_t iv_cap;
    int32_t *state;                 // LOCI_STATE: LOCI_NEXT counts the intervals, LOCI_MAXLEN is their longest
};

__global__ __launch_bounds__(256) void mtr_k_geno_pair(GenoPairArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.rows) return;
    const int rd = (int)(p / a.n_loci), l = (int)(p - (int64_t)rd * a.n_loci);
    const int32_t *f = a.flank + (size_t)p * GT_SLOTS * FL_RES;
    const int32_t *A = f, *B = f + FL_RES, *rA = f + 2 * FL_RES, *rB = f + 3 * FL_RES;
    const bool v0 = A[0] <= a.K && B[0] <= a.K && A[2] <= B[1];
    const bool v1 = rA[0] <= a.K && rB[0] <= a.K && rB[2] <= rA[1];
    const int o = v0 && v1 ? (rA[0] + rB[0] < A[0] + B[0] ? 1 : 0) : v1 ? 1 : 0;
    int32_t *q = a.pair + (size_t)p * GT_PAIR;
    int lo = 0, hi = 0, dl = 0, dr = 0, at = -1;
    if (v0 || v1) {
        dl = o ? rA[0] : A[0]; dr = o ? rB[0] : B[0];
        lo = o ? rB[2] : A[2]; hi = o ? rA[1] : B[1];
        if (hi > lo) {
            at = atomicAdd(&a.state[LOCI_NEXT], 1);
            if (at >= a.iv_cap) { atomicCAS(&a.state[LOCI_STATUS], 0, DEV_ERR_INTERNAL); at = -1; }
            else { a.iv[at] = { rd * (2 * a.n_loci) + 2 * l + o, lo, hi, 0 }; atomicMax(&a.state[LOCI_MAXLEN], hi - lo); }
        }
    }
    q[0] = v0 || v1 ? 1 : 0; q[1] = o; q[2] = dl; q[3] = dr; q[4] = lo; q[5] = hi; q[6] = at; q[7] = 0;
}

struct GenotypesOut { uint8_t *spanning, *orientation; int32_t *flank_dist, *window, *fields, *score; float *ratio; };
// res: the intervals' hits in window coordinates ([interval][MS_RES]); a pair without an interval - not spanning, or an empty window - has zeros
__global__ __launch_bounds__(256) void mtr_k_geno_out(const int32_t *pair, const int32_t *res, int64_t rows, GenotypesOut out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows) return;
    const int32_t *q = pair + (size_t)p * GT_PAIR;
    out.spanning[p] = (uint8_t)q[0]; out.orientation[p] = (uint8_t)q[1];
    out.flank_dist[2 * p] = q[2]; out.flank_dist[2 * p + 1] = q[3];
    out.window[2 * p] = q[4]; out.window[2 * p + 1] = q[5];
    int32_t *o = out.fields + (size_t)p * 8;
    if (q[6] < 0) {
        for (int k = 0; k < 8; k++) o[k] = 0;
        out.score[p] = 0; out.ratio[p] = 0.0f;
        return;
    }
    const int32_t *f = res + (size_t)q[6] * MS_RES;
    o[0] = f[0] + q[4]; o[1] = f[1] + q[4];
    for (int k = 2; k < 8; k++) o[k] = f[k];
    out.score[p] = f[8];
    out.ratio[p] = f[2] > 0 ? (float)f[4] / (float)f[2] : 0.0f;
}
