// motif_loci.hip.inc — known-motif LOCUS search (mtr_search_motif_loci_device): every place of every given motif in every read of the resident batch,
// by the recursion of motif_loci.h run level by level.  Round d holds the windows of depth d as INTERVALS (pair = read * n_motifs + motif, lo, hi);
// an interval on a strand is a TASK (task = interval * strands + strand) with a result slot of its own (MS_RES values, window coordinates), so the
// order in which anything below is appended or pulled never reaches a result.
//   mtr_k_loci_init             round 0: one interval per pair, the whole read.
//   mtr_k_loci_bin              one lane per task.  A task of the lane path (a motif of a lane slot, at most lane_rows rows) counts itself into its BIN
//                               (lane slot, length class: motif_loci.h) and keeps the place it drew there; every other task appends itself to the wave list.
//   mtr_k_loci_groups           a bin of c tasks is ceil(c / 64) GROUPS; mtr_k_scan_offsets (report_align.hip.inc) of the counts and of the groups
//                               gives every bin its first task and its first group.
//   mtr_k_loci_scatter          the tasks into bin order.
//   mtr_k_motif_loci_lanes<UB>  the hot path, as mtr_k_motif_lanes<UB>: ONE WINDOWED DP PER LANE (motif_dp.h with the window's first base).  The lane
//                               slots are numbered bucket by bucket, so a bucket is a range of bins and of groups; a wavefront pulls a group, finds its
//                               bin by bisection on wave-uniform values, and the bin's slot gives the motif: two scalar registers for all 64 lanes, whose
//                               windows are of one length class.  Cells as there: the wavefront's scratch, interleaved by lane.
//   mtr_k_motif_loci_waves      the wave list, one DP per wavefront through dp_wrap(pk, lo - 1, hi - lo, .., mode 0), as mtr_k_motif_waves: row i of the
//                               window is read base lo - 1 + i.  The border is judged by the WINDOW's length: the short children of a long read are lanes' work.
//   mtr_k_loci_split            one lane per interval: the strand by the search's rule, then motif_loci.h's mlo_split - the hit appended to the hit list in
//                               read coordinates, the children to the next round's intervals, the pair's open flag set.
//   mtr_k_loci_count / _starts / _place   the finish: every hit draws a place among its pair's, the counts are scanned into loci_off, the starts go to
//                               their pair's segment, and every hit counts the starts of its segment below its own: its rank, where its columns go.
// What the host reads is LOCI_STATE: once per round the number of intervals the next one has and their longest, so that it can size that round.
#pragma once
#include "motif_search.hip.inc"
#include "motif_loci.h"

enum { LOCI_HITS = 0, LOCI_STATUS, LOCI_NEXT, LOCI_WAVE, LOCI_MAXLEN, LOCI_STATE };      // int32 each; the last three start every round at 0
#define LOCI_HIT 12                 // int32 per hit of the list: pair, the eight fields, score, strand, the place it drew among its pair's

struct LociIv { int32_t pair, lo, hi, pad; };
struct LociArgs {
    BatchView b;
    const LociIv *iv; int32_t n_iv;                                          // this round's intervals
    int32_t n_motifs, n_strands, G, MM, D, lane_rows;
    const uint8_t *units; const int32_t *unit_off; const uint64_t *bits;    // per slot (motif * strands + strand), as the search's
    const int32_t *slot_q, *q_slot;                                          // slot -> its number among the lane slots (-1: none), and back
    int32_t *hist, *groups; int64_t *tfirst, *gfirst; int32_t n_bins;        // per bin
    int32_t *tbin, *trank, *sorted, *wlist;                                  // per task
    int32_t *res;                                                            // [task][MS_RES]
    int32_t *state;                                                          // LOCI_STATE
    int32_t bin0, bin1; unsigned long long *counter;                         // of one launch: its bins, its item counter
    uint8_t *scratch; size_t scratch_per_wave, cells_cap; int32_t dp16_max_rows;
};

__global__ __launch_bounds__(256) void mtr_k_loci_init(const int32_t *lens, int32_t n_motifs, int32_t n_pairs, LociIv *iv)
{
    const int p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p < n_pairs) iv[p] = { p, 0, lens[p / n_motifs], 0 };
}

__global__ __launch_bounds__(256) void mtr_k_loci_bin(LociArgs a)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)a.n_iv * a.n_strands) return;
    const int i = (int)(t / a.n_strands), strand = (int)(t - (long long)i * a.n_strands);
    const LociIv v = a.iv[i];
    const int q = a.slot_q[(v.pair % a.n_motifs) * a.n_strands + strand], len = v.hi - v.lo;
    if (q >= 0 && len <= a.lane_rows) {
        const int bin = q * MLO_N_CLASSES + mlo_len_class(len);
        a.tbin[t] = bin; a.trank[t] = atomicAdd(&a.hist[bin], 1);
    } else {
        a.tbin[t] = -1; a.wlist[atomicAdd(&a.state[LOCI_WAVE], 1)] = (int32_t)t;
    }
}

__global__ __launch_bounds__(256) void mtr_k_loci_groups(const int32_t *hist, int32_t n_bins, int32_t *groups)
{
    const int b = (int)(blockIdx.x * 256 + threadIdx.x);
    if (b < n_bins) groups[b] = (hist[b] + 63) >> 6;
}

__global__ __launch_bounds__(256) void mtr_k_loci_scatter(LociArgs a)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)a.n_iv * a.n_strands) return;
    const int bin = a.tbin[t];
    if (bin >= 0) a.sorted[a.tfirst[bin] + a.trank[t]] = (int32_t)t;
}

template <int UB>
__global__ __launch_bounds__(64) void mtr_k_motif_loci_lanes(LociArgs a)
{
    const int lane = lane_id();
    uint32_t *cells = (uint32_t *)(a.scratch + (size_t)blockIdx.x * a.scratch_per_wave);
    const long long g0 = uni64(a.gfirst[a.bin0]), g1 = uni64(a.gfirst[a.bin1]);
    for (;;) {
        const long long g = g0 + ms_next_item(a.counter);
        if (g >= g1) break;
        int bin = a.bin0, hi = a.bin1;                                           // the last bin whose first group is not beyond g: empty bins share theirs with the next
        while (hi - bin > 1) { const int mid = (bin + hi) >> 1; if (uni64(a.gfirst[mid]) <= g) bin = mid; else hi = mid; }
        const int slot = uni(a.q_slot[bin / MLO_N_CLASSES]);
        const int uo = uni(a.unit_off[slot]), U = uni(a.unit_off[slot + 1]) - uo;
        const uint64_t mot = (uint64_t)uni64((long long)a.bits[slot]);
        const long long at = uni64(a.tfirst[bin]) + (g - uni64(a.gfirst[bin])) * 64 + lane;      // this lane's task of the bin
        const bool has = at < uni64(a.tfirst[bin + 1]);
        int t = 0, lo = 0, L = 0;
        const uint32_t *pk = a.b.packed;
        if (has) {
            t = a.sorted[at];
            const LociIv v = a.iv[t / a.n_strands];
            lo = v.lo; L = v.hi - v.lo; pk = a.b.packed + a.b.woff[v.pair / a.n_motifs];
        }
        const int nd = mdp_dwords(U);
        if ((size_t)L * (size_t)nd * 256 > a.scratch_per_wave || U < 1 || U > UB) { L = 0; atomicCAS(&a.state[LOCI_STATUS], 0, DEV_ERR_INTERNAL); }   // (the host sized the scratch for this)
        const MdpCellsLane c = { cells, nd, lane };
        const MotifHit h = motif_dp<UB>(pk, L, mot, U, a.G, a.MM, a.D, c, lo);
        if (h.score < 0) atomicCAS(&a.state[LOCI_STATUS], 0, DEV_ERR_INTERNAL);
        if (has) {
            int32_t *o = a.res + (size_t)t * MS_RES;
            o[0] = h.start; o[1] = h.end; o[2] = h.repeat_len; o[3] = h.copies; o[4] = h.mat; o[5] = h.mis; o[6] = h.ins; o[7] = h.del;
            o[8] = h.score < 0 ? 0 : h.score;
        }
        loop_join();
    }
}

__global__ __launch_bounds__(64) void mtr_k_motif_loci_waves(LociArgs a)
{
    __shared__ unsigned long long s_cnt[CNT_N];
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    uint8_t *sc = a.scratch + (size_t)blockIdx.x * a.scratch_per_wave;
    const long long n = uni(a.state[LOCI_WAVE]);
    for (;;) {
        const long long w = ms_next_item(a.counter);
        if (w >= n) break;
        const int t = uni(a.wlist[w]);
        const int i = t / a.n_strands, strand = t - i * a.n_strands;
        const int pair = uni(a.iv[i].pair), lo = uni(a.iv[i].lo), len = uni(a.iv[i].hi) - lo;
        const int rd = pair / a.n_motifs, slot = (pair - rd * a.n_motifs) * a.n_strands + strand;
        const int uo = uni(a.unit_off[slot]), U = uni(a.unit_off[slot + 1]) - uo;
        const uint32_t *pk = a.b.packed + uni64(a.b.woff[rd]);
        DpRes o;
        const bool ok = dp_wrap(pk, lo - 1, len, a.units + uo, U, a.G, a.MM, a.D, sc, a.cells_cap, 0, nullptr, nullptr, nullptr, o, s_cnt, a.dp16_max_rows);
        if (!ok) set_status(&a.state[LOCI_STATUS], DEV_ERR_DP_TOO_LARGE);
        if (lane_id() == 0) {
            int32_t *r = a.res + (size_t)t * MS_RES;
            r[0] = o.stop_i; r[1] = o.end_i - 1; r[2] = o.end_i - o.stop_i; r[3] = U > 0 ? o.scanned / U : 0;
            r[4] = o.mat; r[5] = o.mis; r[6] = o.ins; r[7] = o.del;
            r[8] = a.G * o.mat - a.MM * o.mis - a.D * (o.ins + o.del);
        }
        loop_join();
    }
}

// depth: of these intervals; next / hits: the lists they append to, of next_cap intervals and hits_cap hits
__global__ __launch_bounds__(256) void mtr_k_loci_split(LociArgs a, int32_t min_score, int32_t minlen, int32_t rounds, int32_t depth,
                                                        LociIv *next, int32_t next_cap, int32_t *hits, int32_t hits_cap, uint8_t *open)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= a.n_iv) return;
    const LociIv v = a.iv[i];
    const int32_t *f = a.res + (size_t)i * (size_t)a.n_strands * MS_RES;
    int strand = 0;
    if (a.n_strands == 2 && f[MS_RES + 8] > f[8]) { strand = 1; f += MS_RES; }         // (mtr_k_motif_pack's rule)
    const MloSplit s = mlo_split(v.lo, v.hi, depth, rounds, minlen, min_score, f[8], f[0], f[1]);
    if (!s.emit) return;
    const int h = atomicAdd(&a.state[LOCI_HITS], 1);
    if (h >= hits_cap) { atomicCAS(&a.state[LOCI_STATUS], 0, DEV_ERR_INTERNAL); return; }
    int32_t *o = hits + (size_t)h * LOCI_HIT;
    o[0] = v.pair; o[1] = f[0] + v.lo; o[2] = f[1] + v.lo;
    for (int k = 2; k < 8; k++) o[1 + k] = f[k];
    o[9] = f[8]; o[10] = strand; o[11] = 0;
    if (s.open) open[v.pair] = 1;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (k >= s.n) break;
        const int at = atomicAdd(&a.state[LOCI_NEXT], 1);
        if (at >= next_cap) { atomicCAS(&a.state[LOCI_STATUS], 0, DEV_ERR_INTERNAL); return; }
        next[at] = { v.pair, s.clo[k], s.chi[k], 0 };
        atomicMax(&a.state[LOCI_MAXLEN], s.chi[k] - s.clo[k]);
    }
}

// ---- the finish -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mtr_k_loci_count(int32_t *hits, int32_t n_hits, int32_t *count)
{
    const int h = (int)(blockIdx.x * 256 + threadIdx.x);
    if (h < n_hits) hits[(size_t)h * LOCI_HIT + 11] = atomicAdd(&count[hits[(size_t)h * LOCI_HIT]], 1);
}
__global__ __launch_bounds__(256) void mtr_k_loci_starts(const int32_t *hits, int32_t n_hits, const int64_t *loci_off, int32_t *starts)
{
    const int h = (int)(blockIdx.x * 256 + threadIdx.x);
    if (h >= n_hits) return;
    const int32_t *f = hits + (size_t)h * LOCI_HIT;
    starts[loci_off[f[0]] + f[11]] = f[1];
}
struct MotifLociOut { int32_t *fields, *score; float *ratio; uint8_t *strand; };
// Loci of a pair do not overlap, so their starts differ and the rank is a place of its own.  (A hit reads its whole segment: a pair of k loci costs
// k * k loads - DESIGN.md 7i-4.)
__global__ __launch_bounds__(256) void mtr_k_loci_place(const int32_t *hits, int32_t n_hits, const int64_t *loci_off, const int32_t *starts, MotifLociOut out)
{
    const int h = (int)(blockIdx.x * 256 + threadIdx.x);
    if (h >= n_hits) return;
    const int32_t *f = hits + (size_t)h * LOCI_HIT;
    const int64_t s0 = loci_off[f[0]], s1 = loci_off[f[0] + 1];
    int64_t at = s0;
    for (int64_t k = s0; k < s1; k++) at += starts[k] < f[1] ? 1 : 0;
    for (int k = 0; k < 8; k++) out.fields[(size_t)at * 8 + k] = f[1 + k];
    out.score[at] = f[9];
    out.ratio[at] = f[3] > 0 ? (float)f[5] / (float)f[3] : 0.0f;
    out.strand[at] = (uint8_t)f[10];
}
