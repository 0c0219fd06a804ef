// catalog.hip.inc — the catalogue genotype (mtr_genotype_catalog_device): the locus genotype's rows where spanning = 1, for a locus list too long to
// scan every read against every flank.  seed_index.h's pigeonhole screen comes first: an orientation of a (read, locus) whose two flank patterns
// do not BOTH have a seed in the read cannot be valid, so only the others - the CANDIDATES - are verified, by the flank search's own scan
// (flank_bv.h, unchanged) and the genotype's own pairing rule and alignment path.  Nothing here is sized reads x loci.
//   mtr_k_cat_scan       the hot path: one wavefront per read, 64 positions a step.  A lane takes the q-mer at its position out of the packed
//                        words, asks the filter bitmap (a "no" - nearly always - ends the lane's step without a store or a look at the table),
//                        then probes the table.  The lanes of a step that hold the same seed emit it once; the step's entries (locus * 4 +
//                        slot) are placed by a wave scan of the lanes' counts, so that a read's hit list is in the order of its positions:
//                        no atomic decides where anything lands.  Two passes (fill = 0: the read's number of hits; fill = 1: the hits, from
//                        the scanned offsets) - a read may hold any number of hits, nothing is staged at a fixed size.
//   mtr_k_cat_cands      one wavefront per read over its hit list: a hit is a candidate's head if it is slot A or rc A, the first of its key
//                        in the list, and the list holds the partner slot (B or rc B) of its locus.  fill = 0: the heads flagged and counted;
//                        fill = 1: every head at its rank among the read's heads by key - candidates in (read, locus, orientation) order.
//   mtr_k_cat_flank<W>   ONE SCAN PER LANE (fbv_search<W>, as mtr_k_flank_lanes<W> runs it) over the tasks (candidate, side): the task's read
//                        against the task's slot, whose eight masks the lane loads for itself.  Both widths are launched over the same list
//                        and a lane sits out the launch its pattern does not belong to.
//   mtr_k_cat_pair       one lane per candidate; the first candidate of a (read, locus) applies mtr_k_geno_pair's rule with a missing
//                        orientation counted as invalid, and appends the interval with the dense call's pair id.
//   mtr_k_cat_out        the spanning pairs at their scanned places: read, locus and mtr_k_geno_out's seven columns.
//   mtr_k_cat_rows_check the allele calls' check of a row list's read and locus columns (at the end of this file).
#pragma once
#include "genotype.hip.inc"
#include "seed_index.h"

// The filter: 16 bits per distinct seed, between 4 KiB (a small catalogue's stays in a CU's 32 KiB L1) and 2 MiB (half of an XCD's 4 MiB L2, which
// the reads stream through as well); beyond 2^20 seeds the filter fills up and more positions go on to the table.
#define CAT_FILTER_MIN_BITS 15
#define CAT_FILTER_MAX_BITS 24

struct CatScanArgs {
    BatchView b; SiTable ix; const int32_t *ent; int32_t q, fill;
    int32_t *hit_count;                 // per read, saturating at 2^31 - 1: the host refuses a sum that reaches it
    const int64_t *hit_off; int32_t *hits;
    unsigned long long *passed;         // positions the filter let through, counted in the first pass (mtr_test_catalog_stats hands it out)
};

struct SiLoadGlobal { const uint32_t *pk; DEVINL uint32_t operator()(int w) const { return pk[w]; } };

__global__ __launch_bounds__(64) void mtr_k_cat_scan(CatScanArgs a)
{
    const int lane = lane_id();
    const int rd = (int)blockIdx.x;
    if (rd >= a.b.n_reads) return;
    const int n_pos = a.b.lens[rd] - a.q + 1;
    const SiLoadGlobal ld = { a.b.packed + a.b.woff[rd] };
    const int64_t out0 = a.fill ? a.hit_off[rd] : 0;
    long long total = 0;                // (64 bits: a low-complexity seed shared by many loci, in a long read of that repeat, passes 2^31 hits)
    int passed = 0;
    for (int base = 0; base < n_pos; base += 64) {
        const int p = base + lane;
        uint32_t code = 0;
        SiRun run = { 0, 0 };
        if (p < n_pos) {
            code = si_window_code(ld, p, a.q);
            if (si_filter_has(a.ix, code)) { passed++; run = si_probe(a.ix, code); }
        }
        unsigned long long todo = __ballot(run.count > 0);
        if (todo) {
            // one lane per distinct seed of the step
            for (unsigned long long m = todo; m;) {
                const int l = first_lane(m);
                const uint32_t c = (uint32_t)lane_val((int)code, l);
                const unsigned long long same = __ballot(run.count > 0 && code == c);
                if (lane != l && ((same >> lane) & 1ull)) run.count = 0;
                m &= ~same;
            }
            int incl = run.count;
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
            if (a.fill)
                for (int k = 0; k < run.count; k++) a.hits[out0 + total + incl - run.count + k] = a.ent[run.first + k];
            total += lane_val(incl, 63);
        }
        loop_join();
    }
    if (!a.fill) {
        for (int d = 32; d; d >>= 1) passed += __shfl_down(passed, d, 64);
        if (lane == 0) { a.hit_count[rd] = (int32_t)(total < 0x7fffffffll ? total : 0x7fffffffll); if (passed) atomicAdd(a.passed, (unsigned long long)passed); }
    }
}

struct CatCandArgs {
    int32_t n_reads, fill;
    const int64_t *hit_off; const int32_t *hits; uint8_t *head;
    int32_t *cand_count; const int64_t *cand_off;
    int32_t *cand_read, *cand_key;      // key = locus * 2 + orientation
};

__global__ __launch_bounds__(64) void mtr_k_cat_cands(CatCandArgs a)
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
            const int32_t key = hit[i];
            if (!a.fill) {
                bool first = (key & 1) == 0, partner = false;
                if (first)
                    for (int j = 0; j < h; j++) {
                        const int32_t kj = hit[j];
                        if (kj == key && j < i) { first = false; break; }
                        partner |= kj == key + 1;
                    }
                const bool is = first && partner;
                a.head[h0 + i] = is ? 1 : 0;
                heads += is ? 1 : 0;
            } else if (a.head[h0 + i]) {
                int rank = 0;
                for (int j = 0; j < h; j++) rank += a.head[h0 + j] && hit[j] < key ? 1 : 0;
                const int64_t c = a.cand_off[rd] + rank;
                a.cand_read[c] = rd; a.cand_key[c] = key >> 1;
            }
        }
    }
    if (!a.fill) {
        for (int d = 32; d; d >>= 1) heads += __shfl_down(heads, d, 64);
        if (lane == 0) a.cand_count[rd] = heads;
    }
}

struct CatFlankArgs {
    BatchView b;
    const int32_t *cand_read, *cand_key; int32_t n_tasks;           // task = candidate * 2 + side; its slot = key * 2 + side
    const uint64_t *masks; const int32_t *plen; int32_t all_wide;   // per slot: FL_MASKS masks, the pattern's length; all_wide: MTR_TEST_FLANK_WORD=64
    int32_t *res;                                                   // [task][FL_RES]
    int32_t *status;
};

template <class W>
__global__ __launch_bounds__(64) void mtr_k_cat_flank(CatFlankArgs a)
{
    const int t = (int)(blockIdx.x * 64u + threadIdx.x);
    bool has = t < a.n_tasks;
    int rd = 0, L = 0, m = 1;
    size_t slot = 0;
    const uint32_t *pk = a.b.packed;
    if (has) {
        slot = (size_t)a.cand_key[t >> 1] * 2 + (size_t)(t & 1);
        m = a.plen[slot];
        if (m < 1 || m > FBV_MAX_M) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); m = 1; has = false; }
        else has = (sizeof(W) == 8) == (m > 32 || a.all_wide != 0);
    }
    if (!has) m = 1;                                                // (a lane without a task runs zero columns)
    FbvMasks<W> eq = { 0, 0, 0, 0 }, rev = { 0, 0, 0, 0 };
    if (has) {
        rd = a.cand_read[t >> 1]; L = a.b.lens[rd]; pk = a.b.packed + a.b.woff[rd];
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

struct CatPairArgs {
    const int32_t *cand_read, *cand_key; int32_t n_cand;
    const int32_t *flank;               // [candidate * 2 + side][FL_RES]
    int32_t n_loci, K;
    int32_t *pair;                      // [candidate][GT_PAIR]; a candidate that is not the first of its (read, locus) spans nothing
    int32_t *span;                      // [candidate]: 1 = a row
    LociIv *iv; int32_t iv_cap;
    int32_t *state;                     // LOCI_STATE, as mtr_k_geno_pair's
};

__global__ __launch_bounds__(256) void mtr_k_cat_pair(CatPairArgs a)
{
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= a.n_cand) return;
    const int rd = a.cand_read[c], key = a.cand_key[c], l = key >> 1;
    int32_t *q = a.pair + (size_t)c * GT_PAIR;
    const bool head = c == 0 || a.cand_read[c - 1] != rd || (a.cand_key[c - 1] >> 1) != l;
    if (!head) { for (int k = 0; k < GT_PAIR; k++) q[k] = 0; q[6] = -1; a.span[c] = 0; return; }
    const bool two = c + 1 < a.n_cand && a.cand_read[c + 1] == rd && (a.cand_key[c + 1] >> 1) == l;
    const int c0 = (key & 1) == 0 ? c : -1, c1 = (key & 1) ? c : two ? c + 1 : -1;
    const int32_t *A = a.flank + (size_t)(c0 < 0 ? 0 : c0) * 2 * FL_RES, *B = A + FL_RES;
    const int32_t *rA = a.flank + (size_t)(c1 < 0 ? 0 : c1) * 2 * FL_RES, *rB = rA + FL_RES;
    const bool v0 = c0 >= 0 && A[0] <= a.K && B[0] <= a.K && A[2] <= B[1];
    const bool v1 = c1 >= 0 && rA[0] <= a.K && rB[0] <= a.K && rB[2] <= rA[1];
    const int o = v0 && v1 ? (rA[0] + rB[0] < A[0] + B[0] ? 1 : 0) : v1 ? 1 : 0;
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
    a.span[c] = v0 || v1 ? 1 : 0;
}

struct CatRowsOut { int32_t *read, *locus; GenotypesOut g; };
// res: the intervals' hits in window coordinates, as mtr_k_geno_out takes them; row_off: the exclusive sums of span
__global__ __launch_bounds__(256) void mtr_k_cat_out(const int32_t *cand_read, const int32_t *cand_key, const int32_t *pair, const int32_t *span,
                                                     const int64_t *row_off, const int32_t *res, int32_t n_cand, CatRowsOut out)
{
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= n_cand || !span[c]) return;
    const int64_t p = row_off[c];
    const int32_t *q = pair + (size_t)c * GT_PAIR;
    out.read[p] = cand_read[c]; out.locus[p] = cand_key[c] >> 1;
    out.g.spanning[p] = 1; out.g.orientation[p] = (uint8_t)q[1];
    out.g.flank_dist[2 * p] = q[2]; out.g.flank_dist[2 * p + 1] = q[3];
    out.g.window[2 * p] = q[4]; out.g.window[2 * p + 1] = q[5];
    int32_t *o = out.g.fields + (size_t)p * 8;
    if (q[6] < 0) {
        for (int k = 0; k < 8; k++) o[k] = 0;
        out.g.score[p] = 0; out.g.ratio[p] = 0.0f;
        return;
    }
    const int32_t *f = res + (size_t)q[6] * MS_RES;
    o[0] = f[0] + q[4]; o[1] = f[1] + q[4];
    for (int k = 2; k < 8; k++) o[k] = f[k];
    out.g.score[p] = f[8];
    out.g.ratio[p] = f[2] > 0 ? (float)f[4] / (float)f[2] : 0.0f;
}

// mtr_call_alleles_rows_device's check of its two index columns, before any kernel sees the caller's destination: a lane per row.  A read below 0
// or a locus outside 0 .. n_loci - 1 leaves the smallest such row in state[0]; every other row puts its key locus << 32 | read into an
// open-addressing set of cap slots (a power of two, at least twice the rows, all ones = empty), and a key that is already there leaves the smallest
// such key in state[1].  Which of two equal rows finds the other depends on the schedule; whether one does, and the smallest key, do not.
__global__ __launch_bounds__(256) void mtr_k_cat_rows_check(const int32_t *row_read, const int32_t *row_locus, int64_t rows, int32_t n_loci,
                                                            unsigned long long *set, unsigned long long cap, unsigned long long *state)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows) return;
    const int32_t rd = row_read[p], l = row_locus[p];
    if (rd < 0 || l < 0 || l >= n_loci) { atomicMin(&state[0], (unsigned long long)p); return; }
    const unsigned long long key = ((unsigned long long)(uint32_t)l << 32) | (unsigned long long)(uint32_t)rd;
    unsigned long long s = ((unsigned long long)si_hash((uint32_t)l * 0x9E3779B1u ^ (uint32_t)rd)) & (cap - 1);
    for (unsigned long long n = 0; n < cap; n++, s = (s + 1) & (cap - 1)) {
        const unsigned long long was = atomicCAS(&set[s], ~0ull, key);
        if (was == ~0ull) return;
        if (was == key) { atomicMin(&state[1], key); return; }
    }
}
