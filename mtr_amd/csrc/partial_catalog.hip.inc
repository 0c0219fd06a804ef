// partial_catalog.hip.inc — the partial genotype at catalogue scale (mtr_genotype_partial_catalog_device): the rows mtr_genotype_partial_device
// would write with partial = 1, for a locus list too long to scan every read against every flank.  The screen is seed_index.h's, read the other
// way round from the catalogue genotype's: a partial row needs ONE flank within K, a flank within K leaves one of its K + 1 seeds in the read
// verbatim, so the CANDIDATES are the (read, locus) with a seed of ANY of the locus' four slots; a slot without a seed is beyond K whatever a
// scan would say, and is not scanned.  Nothing here is sized reads x loci.  The reads' hit lists are mtr_k_cat_scan's (catalog.hip.inc), unchanged.
//   mtr_k_ptc_cands      one wavefront per read over its hit list (locus * 4 + slot, in position order): a hit is a candidate's head if it is
//                        the first of its LOCUS in the list; the head collects the 4-bit mask of the locus' slots that are in the list.  fill = 0:
//                        the heads' masks stored and the heads counted; fill = 1: every head at its rank among the read's heads by locus -
//                        candidates in (read, locus) order, with their masks and the number of their slots.  The comparison is pairwise, as
//                        quadratic in a read's hits as mtr_k_cat_cands: what that means for q and the catalogue's size is said in include/mtr_hip.h.
//   mtr_k_ptc_tasks      one lane per candidate: its seeded slots as flank tasks (candidate * 4 + slot, UNSIGNED 32 bits: the host admits 2^30 - 1
//                        candidates, whose ids times four pass 2^31) from the scanned offsets, and the entries of its unseeded slots set to a
//                        distance no K reaches.
//   mtr_k_ptc_flank<W>   ONE SCAN PER LANE (fbv_search<W>, unchanged) over the flank tasks; the lane loads its slot's eight masks itself.  Both
//                        widths are launched over the one list and a lane sits out the launch its pattern does not belong to.
//   mtr_k_ptc_pair       one lane per candidate: the genotype's validity test and the partial genotype's choice (partial_choose, the function
//                        mtr_k_partial_pair runs) on the four entries.  A partial candidate with a non-empty window appends a task (candidate,
//                        lo, hi, variant) to the list of its motif's BUCKET: the extension writes at the task's candidate, so the order of the
//                        appends reaches no result.  A flag per candidate feeds the rows' scan.
//   mtr_k_ptc_ext<UB>    the hot path: ONE ANCHORED EXTENSION PER LANE WITH THE MOTIF PER LANE.  A wavefront takes 64 consecutive tasks of its
//                        bucket's list, whatever their loci - in a catalogue a locus meets a handful of reads, and a wavefront per variant
//                        (mtr_k_ext_lanes<UB>) would run a few lanes of 64 - so each lane loads its own motif (a VGPR pair), length and direction
//                        and runs motif_ext_rows<UB, false>: the masked rows are right for every U <= UB, U == UB included, and have no branch
//                        on U or on the direction beyond the word reload.  Nothing is stored per cell: no scratch, no LDS, no cross-lane operation.
//   mtr_k_ptc_out        the partial candidates at their scanned places: read, locus and mtr_k_partial_out's seven columns (partial_row_out).
#pragma once
#include "catalog.hip.inc"
#include "partial.hip.inc"

#define PTC_FAR 0x3fffffff          // the distance of a slot without a seed: beyond every K, and two of them still add up in 32 bits
#define PTC_BUCKETS 4               // the extension's buckets: 4, 8, 16, 32

struct PtcCandArgs {
    int32_t n_reads, fill;
    const int64_t *hit_off; const int32_t *hits; uint8_t *head;         // head: 0 = no head, else the locus' slot mask
    int32_t *cand_count; const int64_t *cand_off;
    int32_t *cand_read, *cand_locus, *cand_mask, *cand_slots;           // cand_slots: the mask's number of bits, the flank tasks' counts
};

__global__ __launch_bounds__(64) void mtr_k_ptc_cands(PtcCandArgs a)
{
    const int lane = lane_id();
    const int rd = (int)blockIdx.x;
    if (rd >= a.n_reads) return;
    const int64_t h0 = a.hit_off[rd];
    const int h = (int)(a.hit_off[rd + 1] - h0);
    const int32_t *hit = a.hits + h0;
    int heads = 0;
    for (int base = 0; base < h; base += 64) {
        const int i = base + lane;
        if (i < h) {
            const int32_t l = hit[i] >> 2;
            if (!a.fill) {
                bool first = true;
                int mask = 0;
                for (int j = 0; j < h; j++) {
                    const int32_t kj = hit[j];
                    if ((kj >> 2) != l) continue;
                    if (j < i) { first = false; break; }
                    mask |= 1 << (kj & 3);
                }
                a.head[h0 + i] = (uint8_t)(first ? mask : 0);
                heads += first ? 1 : 0;
            } else if (a.head[h0 + i]) {
                int rank = 0;
                for (int j = 0; j < h; j++) rank += a.head[h0 + j] && (hit[j] >> 2) < l ? 1 : 0;
                const int64_t c = a.cand_off[rd] + rank;
                const int mask = a.head[h0 + i];
                a.cand_read[c] = rd; a.cand_locus[c] = l; a.cand_mask[c] = mask; a.cand_slots[c] = __popc((unsigned)mask);
            }
        }
    }
    if (!a.fill) {
        for (int d = 32; d; d >>= 1) heads += __shfl_down(heads, d, 64);
        if (lane == 0) a.cand_count[rd] = heads;
    }
}

struct PtcTaskArgs {
    const int32_t *cand_mask; const int64_t *task_off; int32_t n_cand;
    uint32_t *tasks;                    // [flank task] = candidate * 4 + slot, below 2^32 for the 2^30 - 1 candidates the host admits
    int32_t *flank;                     // [candidate][4][FL_RES]
};

__global__ __launch_bounds__(256) void mtr_k_ptc_tasks(PtcTaskArgs a)
{
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= a.n_cand) return;
    const int mask = a.cand_mask[c];
    int64_t at = a.task_off[c];
    for (int s = 0; s < PT_SLOTS; s++) {
        if ((mask >> s) & 1) { a.tasks[at++] = (uint32_t)c * PT_SLOTS + (uint32_t)s; continue; }
        int32_t *o = a.flank + ((size_t)c * PT_SLOTS + (size_t)s) * FL_RES;
        o[0] = PTC_FAR; o[1] = 0; o[2] = 0; o[3] = 0;
    }
}

struct PtcFlankArgs {
    BatchView b;
    const int32_t *cand_read, *cand_locus; int32_t n_cand;                             // (n_cand: a task's candidate is checked against it)
    const uint32_t *tasks; int32_t n_tasks;                                            // task = candidate * 4 + slot (unsigned); its pattern = locus * 4 + slot
    const uint64_t *masks; const int32_t *plen; int32_t all_wide;                      // per pattern: FL_MASKS masks, its length; all_wide: MTR_TEST_FLANK_WORD=64
    int32_t *res;                                                                      // [candidate][4][FL_RES]
    int32_t *status;
};

template <class W>
__global__ __launch_bounds__(64) void mtr_k_ptc_flank(PtcFlankArgs a)
{
    const long long k = (long long)blockIdx.x * 64 + threadIdx.x;
    bool has = k < (long long)a.n_tasks;
    uint32_t t = 0;
    int rd = 0, L = 0, m = 1;
    size_t slot = 0;
    const uint32_t *pk = a.b.packed;
    if (has && (a.tasks[k] >> 2) >= (uint32_t)a.n_cand) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); has = false; }      // (no task names a candidate that is not there)
    if (has) {
        t = a.tasks[k];
        slot = (size_t)a.cand_locus[t >> 2] * PT_SLOTS + (size_t)(t & 3u);
        m = a.plen[slot];
        if (m < 1 || m > FBV_MAX_M) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); m = 1; has = false; }
        else has = (sizeof(W) == 8) == (m > 32 || a.all_wide != 0);
    }
    if (!has) m = 1;                                                // (a lane without a task runs zero columns)
    FbvMasks<W> eq = { 0, 0, 0, 0 }, rev = { 0, 0, 0, 0 };
    if (has) {
        rd = a.cand_read[t >> 2]; L = a.b.lens[rd]; pk = a.b.packed + a.b.woff[rd];
        const uint64_t *mk = a.masks + slot * FL_MASKS;
        eq = { (W)mk[0], (W)mk[1], (W)mk[2], (W)mk[3] };
        rev = { (W)mk[4], (W)mk[5], (W)mk[6], (W)mk[7] };
    }
    const FbvLoadGlobal ld = { pk };
    const FbvHit h = fbv_search<W>(ld, L, eq, rev, m);
    if (!has) return;
    if (h.start < 0) atomicCAS(a.status, 0, DEV_ERR_INTERNAL);
    int32_t *o = a.res + (size_t)t * FL_RES;
    o[0] = h.dist; o[1] = h.start < 0 ? 0 : h.start; o[2] = h.end; o[3] = 0;
}

struct PtcPairArgs {
    const int32_t *cand_read, *cand_locus; int32_t n_cand;
    const int32_t *flank;               // [candidate][4][FL_RES]
    const int32_t *lens, *ulen;         // per read; per locus
    int32_t K;
    int32_t *row;                       // [candidate][PT_ROW], as mtr_k_partial_pair leaves a row
    int32_t *is_row;                    // [candidate]: 1 = a row
    PtTask *tasks;                      // [bucket][n_cand]; a task's row is its candidate
    int32_t *count;                     // [bucket]
    int32_t *status;
};

DEVINL int ptc_bucket_index(int U) { return U <= 4 ? 0 : U <= 8 ? 1 : U <= 16 ? 2 : 3; }      // mdp_bucket(U) = 4 << index

__global__ __launch_bounds__(256) void mtr_k_ptc_pair(PtcPairArgs a)
{
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= a.n_cand) return;
    const int rd = a.cand_read[c], l = a.cand_locus[c];
    const PtChoice ch = partial_choose(a.flank + (size_t)c * PT_SLOTS * FL_RES, a.K, a.lens[rd], a.status);
    int at = -1;
    if (ch.slot >= 0 && ch.hi > ch.lo) {
        const int U = a.ulen[l];
        if (U < 1 || U > MDP_MAX_U) atomicCAS(a.status, 0, DEV_ERR_INTERNAL);
        else {
            const int b = ptc_bucket_index(U);
            at = atomicAdd(&a.count[b], 1);
            if (at >= a.n_cand) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); at = -1; }
            else a.tasks[(size_t)b * (size_t)a.n_cand + (size_t)at] = { c, ch.lo, ch.hi, partial_variant(l, ch.slot) };
        }
    }
    partial_row_store(a.row + (size_t)c * PT_ROW, ch, at);
    a.is_row[c] = ch.slot >= 0 ? 1 : 0;
}

struct PtcExtArgs {
    BatchView b;
    const int32_t *cand_read;
    const PtTask *tasks; const int32_t *count; int32_t n_cand;      // per bucket: its list of n_cand places, the tasks it holds
    const uint64_t *bits; const int32_t *ulen;                      // per variant: the motif as motif_ext takes it; per locus: its length
    int32_t G, MM, D;
    int32_t *ext;                                                   // [candidate][PT_EXT]
    int32_t *status;
};

template <int UB>
__global__ __launch_bounds__(64) void mtr_k_ptc_ext(PtcExtArgs a)
{
    const int b = ptc_bucket_index(UB);
    const long long k = (long long)blockIdx.x * 64 + lane_id();     // this lane's task of the bucket's list
    PtTask t = { 0, 0, 0, 0 };
    const uint32_t *pk = a.b.packed;
    uint64_t mot = 0;
    int U = 1;
    if (k < (long long)a.count[b]) {
        t = a.tasks[(size_t)b * (size_t)a.n_cand + (size_t)k];
        const int rd = a.cand_read[t.row];
        pk = a.b.packed + a.b.woff[rd];
        U = a.ulen[t.variant >> 2];
        mot = a.bits[t.variant];
        if (t.lo < 0 || t.hi > a.b.lens[rd] || t.lo >= t.hi || U < 1 || U > UB) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); t.lo = t.hi = 0; U = 1; }
    }
    if (t.hi <= t.lo) return;
    const FbvLoadGlobal ld = { pk };
    const MotifExt r = motif_ext_rows<UB, false>(ld, t.lo, t.hi, t.variant & 1, mot, U, a.G, a.MM, a.D);
    int32_t *o = a.ext + (size_t)t.row * PT_EXT;
    o[0] = r.ext_len; o[1] = r.motif_bases; o[2] = r.matches; o[3] = r.score;
}

struct PtcRowsOut { int32_t *read, *locus; PartialOut p; };
struct PtcOutArgs {
    const int32_t *cand_read, *cand_locus, *row, *is_row; const int64_t *row_off; const int32_t *ext, *ulen;
    int32_t n_cand, max_tail;
    PtcRowsOut out;
};

__global__ __launch_bounds__(256) void mtr_k_ptc_out(PtcOutArgs a)
{
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= a.n_cand || !a.is_row[c]) return;
    const int64_t p = a.row_off[c];
    const int l = a.cand_locus[c];
    a.out.read[p] = a.cand_read[c]; a.out.locus[p] = l;
    partial_row_out(a.row + (size_t)c * PT_ROW, a.ext + (size_t)c * PT_EXT, a.ulen[l], a.max_tail, p, a.out.p);
}
