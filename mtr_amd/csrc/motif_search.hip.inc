// motif_search.hip.inc — known-motif search (mtr_search_motifs_device): every given motif aligned to every read of the resident batch by the
// wrap-around DP, on both strands.  A (read, motif, strand) alignment is a TASK; the motif-strand pairs are SLOTS (slot = motif * strands + strand,
// the reverse complement's codes made by the host); the reads are taken in the host's order of descending length (`order`).
//   mtr_k_motif_lanes<UB>  the hot path, motifs of up to MDP_MAX_U bases: ONE DP PER LANE (motif_dp.h, the single definition).  A wavefront pulls a
//                          group of 64 consecutive reads of the order for one slot: the motif is wave-uniform (two scalar registers), the lanes' reads
//                          end within a few rows of each other, the previous DP row is UB registers per lane, the cells go to the wavefront's
//                          scratch interleaved by lane (a store instruction writes 256 contiguous bytes), and each lane walks its own traceback.
//                          No cross-lane operation between the pull and loop_join(): a lane without a task (the last group of a slot) runs zero
//                          rows on a full wave.
//   mtr_k_motif_waves      everything else - longer motifs, and reads beyond the lane path's row bound: one DP per wavefront through dp_wrap(mode 0),
//                          as mtr_k_dp_test, with the tasks made here from the work list.  The whole read is the window base = -1, rows = L:
//                          rep[i] = x[i - 1].  Every forward pass of dp_wrap reads the word of position base + i >= 0 (dp_forward<NCH> and
//                          dp_forward_2c: blk = (base + i) >> 10; dp_forward1p_g16: pos0 = base + 1 + t0, clamped to [0, wlim)), and the mode-0
//                          traceback reads no base at all (only MODE 1 does), so no variant loads below the read's first word.  dp_wrap does
//                          not return the best cell's value: the score is the identity G * mat - MM * mis - D * (ins + del), exact because
//                          the traceback ends on a cell of value 0 or in row 0.
//   mtr_k_motif_pack       picks the strand (the higher score, the forward motif on a tie) and writes the caller's columns at read * n_motifs + motif.
// A work list (MsWork) is what one launch pulls from: entries (slot, first item), items numbered through; the entry of an item is found by
// bisection on wave-uniform values.  The item counter is 64-bit: 2^31 - 1 hits on two strands are more than 2^32 tasks.
#pragma once
#include "dp_wrap.hip.inc"
#include "motif_dp.h"

#define MS_RES 9                    // int32 per task: the eight fields and the score
#define MS_LANE_MAX_U 16            // the longest motif the lane path takes by default (DESIGN.md 7i-3: the measurement that chose it)
#define MS_LANE_ROWS 16384          // reads of more bases take the wave path: a lane's cells are 256 bytes apart, 64 of them a row-dword of the wavefront -
                                    // 16384 rows of a 16-base motif are 16 MB of scratch per wavefront (the search's host side sizes it by the longest lane read)

struct MsWork { const int32_t *slot; const int64_t *first; int32_t n_entries; int64_t n_items; };
struct MotifSearchArgs {
    BatchView b;
    const int32_t *order;           // reads by descending length
    int32_t n_reads, n_long;        // the first n_long reads of the order exceed the lane path's rows
    const uint8_t *units; const int32_t *unit_off; const uint64_t *bits;      // per slot: its codes, and for U <= MDP_MAX_U the 2-bit form
    int32_t n_motifs, n_strands, G, MM, D;
    int32_t *res;                   // [(read * n_motifs + motif) * n_strands + strand][MS_RES]
    MsWork work; unsigned long long *counter;
    uint8_t *scratch; size_t scratch_per_wave; size_t cells_cap;
    int32_t *status; int32_t dp16_max_rows;
};

DEVINL long long ms_next_item(unsigned long long *counter)
{
    unsigned long long t = 0;
    if (lane_id() == 0) t = atomicAdd(counter, 1ull);
    unsigned lo = (unsigned)t, hi = (unsigned)(t >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));                 // (next_work_item's hazard: lanes 1..63 must not be known to hold 0)
    return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)hi) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)lo));
}
// the entry e with first[e] <= item < first[e + 1] (first[n_entries] = n_items); wave-uniform
DEVINL int ms_entry(const MsWork &w, long long item)
{
    int lo = 0, hi = w.n_entries;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (uni64(w.first[mid]) <= item) lo = mid; else hi = mid; }
    return lo;
}
DEVINL int32_t *ms_res(const MotifSearchArgs &a, int rd, int slot)
{
    const int motif = slot / a.n_strands, strand = slot - motif * a.n_strands;
    return a.res + (((size_t)rd * (size_t)a.n_motifs + (size_t)motif) * (size_t)a.n_strands + (size_t)strand) * MS_RES;
}

template <int UB>
__global__ __launch_bounds__(64) void mtr_k_motif_lanes(MotifSearchArgs a)
{
    const int lane = lane_id();
    uint32_t *cells = (uint32_t *)(a.scratch + (size_t)blockIdx.x * a.scratch_per_wave);
    for (;;) {
        const long long g = ms_next_item(a.counter);
        if (g >= a.work.n_items) break;
        const int e = ms_entry(a.work, g);
        const int slot = uni(a.work.slot[e]);
        const int uo = uni(a.unit_off[slot]), U = uni(a.unit_off[slot + 1]) - uo;
        const uint64_t mot = (uint64_t)uni64((long long)a.bits[slot]);
        const long long r = (long long)a.n_long + (g - uni64(a.work.first[e])) * 64 + lane;      // this lane's read of the order
        const bool has = r < (long long)a.n_reads;
        int rd = 0, L = 0;
        const uint32_t *pk = a.b.packed;
        if (has) { rd = a.order[r]; L = a.b.lens[rd]; pk = a.b.packed + a.b.woff[rd]; }
        const int nd = mdp_dwords(U);
        if ((size_t)L * (size_t)nd * 256 > a.scratch_per_wave || U < 1 || U > UB) { L = 0; atomicCAS(a.status, 0, DEV_ERR_INTERNAL); }    // (the host sized the scratch for this)
        const MdpCellsLane c = { cells, nd, lane };
        const MotifHit h = motif_dp<UB>(pk, L, mot, U, a.G, a.MM, a.D, c);
        if (h.score < 0) atomicCAS(a.status, 0, DEV_ERR_INTERNAL);
        if (has) {
            int32_t *o = ms_res(a, rd, slot);
            o[0] = h.start; o[1] = h.end; o[2] = h.repeat_len; o[3] = h.copies; o[4] = h.mat; o[5] = h.mis; o[6] = h.ins; o[7] = h.del;
            o[8] = h.score < 0 ? 0 : h.score;
        }
        loop_join();
    }
}

__global__ __launch_bounds__(64) void mtr_k_motif_waves(MotifSearchArgs a)
{
    __shared__ unsigned long long s_cnt[CNT_N];
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    uint8_t *sc = a.scratch + (size_t)blockIdx.x * a.scratch_per_wave;
    for (;;) {
        const long long t = ms_next_item(a.counter);
        if (t >= a.work.n_items) break;
        const int e = ms_entry(a.work, t);
        const int slot = uni(a.work.slot[e]);
        const int uo = uni(a.unit_off[slot]), U = uni(a.unit_off[slot + 1]) - uo;
        const int rd = uni(a.order[t - uni64(a.work.first[e])]);
        const int L = uni(a.b.lens[rd]);
        const uint32_t *pk = a.b.packed + uni64(a.b.woff[rd]);
        DpRes o;
        const bool ok = dp_wrap(pk, -1, L, a.units + uo, U, a.G, a.MM, a.D, sc, a.cells_cap, 0, nullptr, nullptr, nullptr, o, s_cnt, a.dp16_max_rows);
        if (!ok) set_status(a.status, DEV_ERR_DP_TOO_LARGE);
        if (lane_id() == 0) {
            int32_t *r = ms_res(a, rd, slot);
            r[0] = o.stop_i; r[1] = o.end_i - 1; r[2] = o.end_i - o.stop_i; r[3] = U > 0 ? o.scanned / U : 0;
            r[4] = o.mat; r[5] = o.mis; r[6] = o.ins; r[7] = o.del;
            r[8] = a.G * o.mat - a.MM * o.mis - a.D * (o.ins + o.del);
        }
        loop_join();
    }
}

struct MotifHitsOut { int32_t *fields, *score; float *ratio; uint8_t *strand; };
__global__ __launch_bounds__(256) void mtr_k_motif_pack(const int32_t *res, int32_t n_strands, int64_t n_hits, MotifHitsOut out)
{
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= n_hits) return;
    const int32_t *f = res + (size_t)h * (size_t)n_strands * MS_RES;
    int strand = 0;
    if (n_strands == 2 && f[MS_RES + 8] > f[8]) { strand = 1; f += MS_RES; }
    for (int k = 0; k < 8; k++) out.fields[(size_t)h * 8 + k] = f[k];
    out.score[h] = f[8];
    out.ratio[h] = f[2] > 0 ? (float)f[4] / (float)f[2] : 0.0f;
    out.strand[h] = (uint8_t)strand;
}
