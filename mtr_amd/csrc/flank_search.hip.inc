// flank_search.hip.inc — flank search (mtr_search_flanks_device, and the first step of mtr_genotype_loci_device): every given pattern of up to 64
// bases matched approximately against every read of the resident batch.  A (read, pattern-strand) match is a TASK; the pattern-strand pairs are
// SLOTS (the host makes the reverse complement's masks); the reads are taken in the host's order of descending length, as the known-motif search's.
//   mtr_k_flank_lanes<W>   ONE SCAN PER LANE in Myers' bit-vector form (flank_bv.h, the single definition).  A wavefront pulls a group of 64
//                          consecutive reads of the order for one slot: the slot's eight match masks (the pattern's and the reversed pattern's,
//                          four each) are wave-uniform - scalar registers - and the lanes' reads end within a few columns of each other.  A lane
//                          keeps the two delta vectors, the running score, the best score and its end, and loads one word of its own read per 16
//                          bases; after the forward scan it runs the anchored backward scan for the start, at most m + dist columns.  W is the
//                          word: uint32_t for patterns of up to 32 bases, uint64_t beyond; one launch per width over the slots that fall into it.
//                          No cells, no traceback: no scratch, no LDS.  No cross-lane operation between the pull and loop_join(): a lane without
//                          a task (the last group of a slot) runs zero columns on a full wave.
//   mtr_k_flank_pack       picks the strand (the smaller distance, the forward pattern on a tie) and writes the caller's columns at
//                          read * n_patterns + pattern.
// The per-slot results (FL_RES values at read * n_slots + slot) stay where the lanes wrote them: the genotype pairs them before any strand is picked.
#pragma once
#include "motif_search.hip.inc"
#include "flank_bv.h"

#define FL_RES 4                    // int32 per task: dist, start, end, and a spare
#define FL_MASKS 8                  // 64-bit values per slot: the masks of A, C, G, T of the pattern, then of the reversed pattern

struct FlankArgs {
    BatchView b;
    const int32_t *order;           // reads by descending length
    int32_t n_reads, n_slots;
    const uint64_t *masks; const int32_t *plen;         // per slot: FL_MASKS masks, the pattern's length
    int32_t *res;                   // [read * n_slots + slot][FL_RES]
    MsWork work; unsigned long long *counter;
    int32_t *status;
};

struct FbvLoadGlobal { const uint32_t *pk; DEVINL uint32_t operator()(int w) const { return pk[w]; } };

template <class W>
__global__ __launch_bounds__(64) void mtr_k_flank_lanes(FlankArgs a)
{
    const int lane = lane_id();
    for (;;) {
        const long long g = ms_next_item(a.counter);
        if (g >= a.work.n_items) break;
        const int e = ms_entry(a.work, g);
        const int slot = uni(a.work.slot[e]);
        const int m = uni(a.plen[slot]);
        const uint64_t *mk = a.masks + (size_t)slot * FL_MASKS;
        const FbvMasks<W> eq = { (W)uni64((long long)mk[0]), (W)uni64((long long)mk[1]), (W)uni64((long long)mk[2]), (W)uni64((long long)mk[3]) };
        const FbvMasks<W> rev = { (W)uni64((long long)mk[4]), (W)uni64((long long)mk[5]), (W)uni64((long long)mk[6]), (W)uni64((long long)mk[7]) };
        const long long r = (g - uni64(a.work.first[e])) * 64 + lane;                             // this lane's read of the order
        const bool has = r < (long long)a.n_reads;
        int rd = 0, L = 0;
        const uint32_t *pk = a.b.packed;
        if (has) { rd = a.order[r]; L = a.b.lens[rd]; pk = a.b.packed + a.b.woff[rd]; }
        const bool fits = m >= 1 && m <= (int)(8 * sizeof(W));                                   // (the host sorted the slots by this)
        if (!fits) { L = 0; atomicCAS(a.status, 0, DEV_ERR_INTERNAL); }
        const FbvLoadGlobal ld = { pk };
        const FbvHit h = fbv_search<W>(ld, L, eq, rev, fits ? m : 1);
        if (h.start < 0) atomicCAS(a.status, 0, DEV_ERR_INTERNAL);
        if (has) {
            int32_t *o = a.res + ((size_t)rd * (size_t)a.n_slots + (size_t)slot) * FL_RES;
            o[0] = h.dist; o[1] = h.start < 0 ? 0 : h.start; o[2] = h.end; o[3] = 0;
        }
        loop_join();
    }
}

struct FlankHitsOut { int32_t *dist, *start, *end; uint8_t *strand; };
__global__ __launch_bounds__(256) void mtr_k_flank_pack(const int32_t *res, int32_t n_strands, int64_t n_hits, FlankHitsOut out)
{
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= n_hits) return;
    const int32_t *f = res + (size_t)h * (size_t)n_strands * FL_RES;
    int strand = 0;
    if (n_strands == 2 && f[FL_RES] < f[0]) { strand = 1; f += FL_RES; }
    out.dist[h] = f[0]; out.start[h] = f[1]; out.end[h] = f[2];
    out.strand[h] = (uint8_t)strand;
}
