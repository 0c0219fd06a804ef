// allele_call.hip.inc — allele calls per locus (mtr_call_alleles_device; mtr_call_alleles_rows_device: the same over a list of rows that name
// their read and locus): genotype rows [read][locus] in device memory reduced to one row per
// locus - the supporting reads ranked by (value, read), and the ranked list split into one or two alleles.  The definition is
// include/mtr_hip.h's ("allele calls"); the split itself is allele_split.h, shared with the host.  Five launches on the context's stream, no
// waiting between workgroups, every output an exact integer:
//   mtr_k_allele_count    one lane per row: a supporting row adds 1 to its locus' counter; a supporting row of negative value leaves the smallest
//                         such row in the state
//   mtr_k_allele_offsets  one wavefront: the exclusive scans of the counts (support_off) and of ceil(S_l / TILE) (the rank's tile list), S, the
//                         number of tiles
//   mtr_k_allele_fill     one lane per row: a supporting row takes a slot of its locus' segment through a cursor and leaves the key
//                         value << 32 | read there.  The order of the slots reaches no result
//   mtr_k_allele_rank     one workgroup per (locus, tile of TILE members), found by a binary search over the tile list as pack.hip.inc searches
//                         woff: each lane holds one key, the locus' whole key list streams through LDS, the lane counts the keys smaller than
//                         its own ("counting the smaller ones", chain.hip.inc) - the keys are distinct, so the counts are a permutation - and
//                         writes value and read at its rank
//   mtr_k_allele_split    one workgroup per locus: int64 prefix sums of the sorted values into the context's buffer, each lane its share of the
//                         splits (allele_split.h), the lexicographic minimum of (cost2, k) over the workgroup, the locus' outputs and allele[]
// Counter and cursor: with fewer loci than lanes a wavefront's rows share few counters, so the lanes of one locus are counted by a ballot and
// ONE lane adds their number (one atomic per wavefront and locus, not 64 on one address); from 64 loci on every lane adds for itself, and up to
// AL_SPREAD_LOCI loci the counters lie 256 bytes apart: 64 neighbouring counters are two cache lines, on which the atomics queue.
#pragma once
#include "device_util.hip.inc"
#include "allele_split.h"

#define AL_TILE 256                 // members of one rank tile = lanes of its workgroup = keys of one LDS chunk
#define AL_BLOCK 256                // lanes of the per-row kernels and of the split's workgroup
#define AL_STATE 4                  // int64: the smallest supporting row of negative value (-1 as unsigned: none), S, the number of tiles, a spare
#define AL_BAD 0
#define AL_TOTAL 1
#define AL_TILES 2
#define AL_SPREAD 64                // int32 between two loci's counters while the loci are few: atomics on one cache line complete one after the other
#define AL_SPREAD_LOCI 4096         // (tests/dev/atomic_rate.hip, device_util.hip.inc), 256 bytes apart side by side; more loci than this spread by themselves
#define AL_MAX_GRID (1 << 20)       // workgroups of the rank and of the split; more items than this are strided over

struct AlleleArgs {
    const uint8_t *spanning; const int32_t *window, *fields; const float *ratio;        // the genotype's columns, row = read * n_loci + locus
    const int32_t *row_read, *row_locus;                                                // or NULL: rows in any order, each with its read and locus (mtr_call_alleles_rows_device)
    int64_t rows; int32_t n_loci, measure; float min_ratio; AlleleRule rule;
    int32_t *count, *cursor;        // [n_loci * cstride] each, zeroed by the host: locus l's at l * cstride
    int32_t cstride;                // AL_SPREAD up to AL_SPREAD_LOCI loci, else 1
    int64_t *off, *tile_off;        // [n_loci + 1] each
    int64_t *state;                 // [AL_STATE]
    unsigned long long *keys;       // [S]: locus l's at off[l] ..
    int64_t *prefix;                // [S + n_loci]: locus l's S_l + 1 prefix sums at off[l] + l ..
    int32_t *value, *read; uint8_t *allele, *zygosity; int32_t *call, *call_support; int64_t *cost;   // the caller's columns
};

// does row p support its locus, and with which value?
DEVINL bool allele_row(const AlleleArgs &a, int64_t p, int32_t &v)
{
    v = 0;
    if (p >= a.rows || a.spanning[p] != 1) return false;
    const int32_t lo = a.window[2 * p], hi = a.window[2 * p + 1];
    if (hi != lo && !(a.ratio[p] >= a.min_ratio)) return false;
    v = a.measure == 0 ? a.fields[8 * p + 3] : hi - lo;
    return true;
}

// the read and the locus of row p < a.rows
DEVINL void allele_where(const AlleleArgs &a, int64_t p, int64_t &rd, int &l)
{
    if (a.row_locus) { rd = a.row_read[p]; l = a.row_locus[p]; }
    else { rd = p / a.n_loci; l = (int)(p - rd * a.n_loci); }
}

// counter[l] += 1 for every lane with take set; returns the counter's value before this lane's own add (what a cursor hands out).  Every lane
// of the wavefront comes here, taking or not.
DEVINL int allele_take(int32_t *counter, int l, bool take, bool few_loci)
{
    if (!few_loci) return take ? atomicAdd(&counter[l], 1) : 0;
    int slot = 0;
    unsigned long long todo = __ballot(take);
    while (todo != 0ull) {                                              // (wave-uniform: one turn per locus among the taking lanes)
        const int lead = first_lane(todo);
        const int ll = bcast(l, lead);
        const bool mine = take && l == ll;
        const unsigned long long same = __ballot(mine);
        int base = 0;
        if (lane_id() == lead) base = atomicAdd(&counter[ll], (int)__popcll(same));
        base = bcast(base, lead);
        if (mine) slot = base + mbcnt(same);
        todo &= ~same;
        loop_join();
    }
    return slot;
}

__global__ __launch_bounds__(AL_BLOCK) void mtr_k_allele_count(AlleleArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * AL_BLOCK + threadIdx.x;
    int32_t v;
    const bool sup = allele_row(a, p, v);
    int64_t rd = 0; int l = 0;
    if (p < a.rows) allele_where(a, p, rd, l);
    if (sup && v < 0) atomicMin((unsigned long long *)&a.state[AL_BAD], (unsigned long long)p);
    (void)allele_take(a.count, l * a.cstride, sup, a.n_loci < 64);
}

__global__ __launch_bounds__(64) void mtr_k_allele_offsets(AlleleArgs a)
{
    const int lane = lane_id();
    long long sum = 0, tiles = 0;                                       // what lies before this turn's 64 loci
    for (int64_t l0 = 0; l0 < a.n_loci; l0 += 64) {
        const int64_t l = l0 + lane;
        const long long c = l < a.n_loci ? a.count[l * a.cstride] : 0, t = (c + AL_TILE - 1) / AL_TILE;
        long long ic = c, it = t;                                       // inclusive scans over the lanes
        for (int d = 1; d < 64; d <<= 1) {
            const long long oc = __shfl_up(ic, d, 64), ot = __shfl_up(it, d, 64);
            if (lane >= d) { ic += oc; it += ot; }
        }
        if (l < a.n_loci) { a.off[l] = sum + ic - c; a.tile_off[l] = tiles + it - t; }
        sum += __shfl(ic, 63, 64); tiles += __shfl(it, 63, 64);
    }
    if (lane == 0) { a.off[a.n_loci] = sum; a.tile_off[a.n_loci] = tiles; a.state[AL_TOTAL] = sum; a.state[AL_TILES] = tiles; }
}

__global__ __launch_bounds__(AL_BLOCK) void mtr_k_allele_fill(AlleleArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * AL_BLOCK + threadIdx.x;
    int32_t v;
    const bool sup = allele_row(a, p, v);
    int64_t rd = 0; int l = 0;
    if (p < a.rows) allele_where(a, p, rd, l);
    const int slot = allele_take(a.cursor, l * a.cstride, sup, a.n_loci < 64);
    if (!sup) return;
    const int64_t at = a.off[l] + slot;
    if (at < a.off[l + 1]) a.keys[at] = ((unsigned long long)(uint32_t)v << 32) | (unsigned long long)(uint32_t)rd;       // (the count and the fill see the same rows)
}

__global__ __launch_bounds__(AL_TILE) void mtr_k_allele_rank(AlleleArgs a, int64_t n_tiles)
{
    __shared__ unsigned long long chunk[AL_TILE];
    const int tid = (int)threadIdx.x;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int64_t lo = 0, hi = (int64_t)a.n_loci - 1;                     // the last locus whose first tile is <= t: loci without support own no tile
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (a.tile_off[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const int64_t base = a.off[lo], S = a.off[lo + 1] - base;
        const int64_t i = (t - a.tile_off[lo]) * AL_TILE + tid;
        const unsigned long long none = ~0ull;                          // above every key: values are >= 0
        const unsigned long long mine = i < S ? a.keys[base + i] : none;
        int64_t rank = 0;
        for (int64_t c = 0; c < S; c += AL_TILE) {
            __syncthreads();                                            // (the previous chunk has been read)
            chunk[tid] = c + tid < S ? a.keys[base + c + tid] : none;
            __syncthreads();
            int smaller = 0;
#pragma unroll 8
            for (int j = 0; j < AL_TILE; j++) smaller += chunk[j] < mine ? 1 : 0;
            rank += smaller;
        }
        if (i < S) { a.value[base + rank] = (int32_t)(mine >> 32); a.read[base + rank] = (int32_t)(uint32_t)mine; }
    }
}

__global__ __launch_bounds__(AL_BLOCK) void mtr_k_allele_split(AlleleArgs a)
{
    __shared__ long long part[AL_BLOCK / 64][2];                        // per wavefront: its sum (the scan), then its best split's (cost, k)
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (int64_t l = blockIdx.x; l < a.n_loci; l += gridDim.x) {
        const int64_t base = a.off[l], S = a.off[l + 1] - base;
        const int32_t *v = a.value + base;
        int64_t *pre = a.prefix + base + l;
        // the prefix sums, AL_BLOCK values a turn
        long long before = 0;
        for (int64_t c = 0; c < S; c += AL_BLOCK) {
            const int64_t i = c + tid;
            long long inc = i < S ? v[i] : 0;
            for (int d = 1; d < 64; d <<= 1) { const long long o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
            __syncthreads();
            if (lane == 63) part[wave][0] = inc;
            __syncthreads();
            long long total = 0;
            for (int w = 0; w < AL_BLOCK / 64; w++) { const long long s = part[w][0]; if (w < wave) inc += s; total += s; }
            if (i < S) pre[i + 1] = before + inc;
            before += total;
        }
        if (tid == 0) pre[0] = 0;
        __syncthreads();                                                // (the workgroup's own stores to pre are visible to all of it)
        // this lane's share of the splits, then the workgroup's best
        const bool called = S >= 1 && S >= (int64_t)a.rule.min_support;
        AlleleSplit best = allele_no_split();
        if (called) best = allele_best_split(v, pre, S, a.rule, 1 + tid, AL_BLOCK);
        for (int d = 32; d > 0; d >>= 1) {
            const long long oc = __shfl_xor((long long)best.cost, d, 64), ok = __shfl_xor((long long)best.k, d, 64);
            if (allele_better(oc, ok, best.cost, best.k)) { best.cost = oc; best.k = ok; }
        }
        if (lane == 0) { part[wave][0] = best.cost; part[wave][1] = best.k; }
        __syncthreads();
        best.cost = part[0][0]; best.k = part[0][1];
        for (int w = 1; w < AL_BLOCK / 64; w++)
            if (allele_better(part[w][0], part[w][1], best.cost, best.k)) { best.cost = part[w][0]; best.k = part[w][1]; }
        __syncthreads();                                                // (part is free for the next locus)
        const int64_t k = best.k;
        if (tid == 0) {
            int32_t c0 = 0, c1 = 0, n0 = 0, n1 = 0; int64_t cost1 = 0, cost2 = 0; uint8_t z = 0;
            if (called) {
                const AlleleSeg all = allele_seg(v, pre, 0, S);
                z = 1; c0 = c1 = all.med; n0 = (int32_t)S; cost1 = cost2 = all.sad;
                if (k > 0) { z = 2; c0 = allele_seg(v, pre, 0, k).med; c1 = allele_seg(v, pre, k, S).med; n0 = (int32_t)k; n1 = (int32_t)(S - k); cost2 = best.cost; }
            }
            a.zygosity[l] = z; a.call[2 * l] = c0; a.call[2 * l + 1] = c1; a.call_support[2 * l] = n0; a.call_support[2 * l + 1] = n1;
            a.cost[2 * l] = cost1; a.cost[2 * l + 1] = cost2;
        }
        for (int64_t i = tid; i < S; i += AL_BLOCK) a.allele[base + i] = k > 0 && i >= k ? 1 : 0;
    }
}
