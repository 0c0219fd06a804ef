// k2_units.hip.inc — the unit phase and the kernels built on it: for every candidate range of a read infer the
// repeat unit and score it.
//
// Replaces handle_one_TR's range loop and everything below it (reference handle_one_read.c:77-261,
// consensus.c:37-1087, wrap_around_DP.c:57-429).  Kernels:
//   mtr_k_reads        one wavefront per read: its ranges (k1_read, k1_ranges.hip.inc), then the reference's sequential
//                      range loop (k2_read) - a reported repeat removes later ranges (handle_one_read.c:242-243);
//   mtr_k_range_units  + mtr_k_replay: the range-parallel mode of small batches (every range is a work item, the
//                      sequential pruning is replayed afterwards);
//   mtr_k_align        the -a alignment paths of reported repeats;
//   mtr_k_dp_test      wrap_around_DP_sub alone (parity tests).
// Inside a range the 64 lanes are used for
//   * the exact k-mer multiset of the window in LDS (direct / packed / split layouts, LDS atomics; consensus.c:62-229
//     semantics: counts, maximum frequency, first-occurrence seed list with the reference's decrement of every
//     listed node);
//   * the greedy De Bruijn walks: the successor look-ups of a step are done by different lanes, the decision is
//     scalar; deeper look-ahead keeps ordered tie lists compacted with ballots (consensus.c:269-505);
//   * the wrap-around DP (dp_wrap.hip.inc);
//   * the per-column votes of the unit revision (consensus.c:964-1012).
// Work whose result is known is not repeated: per-range memo of wrap_around_DP, tables bounded by a smaller k,
// walks that enter a cycle, re-alignments of an unchanged unit (DESIGN.md 4.2).
#pragma once
#include "device_util.hip.inc"
#include "dp_wrap.hip.inc"
#include "min_missing_table.h"
#include "polish_plan.h"

#ifndef MTR_WAVES_PER_SIMD
#define MTR_WAVES_PER_SIMD 4       // 16 wavefronts per CU = 128 VGPRs each (an experiment build may lower it: fewer spills, less latency hiding)
#endif
// The walk and polish kernels wait on memory; their bound leaves each SIMD 128 of its 512 registers beside four of their wavefronts: one DP wavefront of another batch
// in flight.  (Registers only.  LDS is handed out in granules of 1 280 bytes, tests/dev/coresidency_probe.hip: the 10 080-byte arena below takes eight of a CU's 128,
// sixteen wavefronts take them all, and no wavefront that declares any LDS enters beside them until the arena kernels fit seven granules - DESIGN.md 4.11.)
#ifndef MTR_LAT_WAVES_PER_SIMD
#define MTR_LAT_WAVES_PER_SIMD 5
#endif
#define MTR_LDS_PER_CU (160 * 1024)
#define MTR_LDS_GRANULE 1280
#define MTR_LDS_ALLOC(bytes) (((bytes) + MTR_LDS_GRANULE - 1) / MTR_LDS_GRANULE * MTR_LDS_GRANULE)
#define MTR_ARENA_CORESIDENT_BYTES (7 * MTR_LDS_GRANULE)     // what an arena kernel (arena + counters) may declare for four DP wavefronts to fit beside sixteen of its own
#define K2_TAB_CAP 2048            // 32-bit words of the LDS table area (8 KB)
#define K2_TAB_MAX_WIDTH 1400      // windows up to this many positions use the LDS table
#define K2_EMPTY (-1)

__device__ __constant__ char d_min_missing[2001] = MTR_MIN_MISSING_DIGITS_STR;

struct RR {                         // the scalar fields of repeat_in_read (mTR.h:99-119), wave-uniform
    int rep_start, rep_end, repeat_len, period, copies, mat, mis, ins, del, kmer, G, MM, D;
};
DEVINL void rr_clear(RR &r)
{   // clear_rr, fill_directional_index.c:40-60
    r.rep_start = r.rep_end = r.repeat_len = r.period = r.copies = -1;
    r.mat = r.mis = r.ins = r.del = r.kmer = r.G = r.MM = r.D = -1;
}
DEVINL float rr_ratio(const RR &r)
{   // (float)Num_matches / (int sum)  — handle_one_read.c:137, consensus.c:562, wrap_around_DP.c:397
    return (float)r.mat / (float)(r.mat + r.mis + r.ins + r.del);
}

// use_lds: keys in LDS (windows up to K2_TAB_MAX_WIDTH), else in global scratch.  vals_lds: the counts sit in the
// unused upper half of the LDS key array (tables of <= 1024 slots, i.e. windows up to 512 positions - 96 % of all
// tables never touch global memory); else in global scratch.
struct Tab { int fmt; int use_lds; int vals_lds; unsigned mask; unsigned nslots; int *gkeys; int *gvals;
             int n_compact; int *ckeys; int *cslots; };      // a table in global memory: its n_compact distinct keys and their slots, in slot order (else -1)
#define K2_VALS_LDS_OFF 1024

struct K2Ctx {
    const K2Args *a;
    const uint32_t *pk; int L; int rd;
    uint8_t *sc; K2Layout y;
    lds_int *lds_keys, *seeds, *stage;   // LDS: keys of the k-mer table (counts live in global scratch), seed list, 4x64 staging
    int *ties, *fresh;             // tie lists of the look-ahead (global scratch: only the rare wide-tie path uses them)
    unsigned long long *wc;        // this wave's work counters (LDS), flushed to the global ones once per read
    Tab tab; int tab_k;
    // memo of wrap_around_DP results for the current range: lane e keeps the unit length of entry e
    int memo_n, memo_qs, memo_qe, memo_U;
    int rmemo_n;                   // revisions remembered for the current range (revise)
    // the look-ahead's step cache (walk): an entry counts for the table it was written under (tab_gen, one per table built by this wavefront in
    // this kernel) - no clearing per table; sc_ready: bit 0 / 1 = the cache's small / whole region carries no entry of an earlier kernel
    int tab_gen = 0, sc_ready = 0;
    int idx_gen_f = -1, idx_gen_b = -1;   // the table (tab_gen) whose keys are grouped by their first / last five digits right now (idx_build; LDS: the bucket ends).
                                   // (Two scalars: an array indexed by the direction would keep this whole struct in scratch memory)
    bool staged_walks = false;     // the walks of the staged chain: a found unit is copied out by its length (st_park_entries), the slot's tail is not filled
#ifdef MTR_PROFILE_WALK_FMT
    int prof_kernel = 0;           // development build: 1 inside mtr_k_walks_k
#endif
};

// a DP of read c.rd exceeded the reference's WrapDPsize: the reference exits there (wrap_around_DP.c:259-262), having
// printed every read before this one; the host reports the reads before the FIRST such read of the batch
DEVINL void dp_too_large(K2Ctx &c)
{
    set_status(c.a->status, DEV_ERR_DP_TOO_LARGE);
    if (lane_id() == 0 && c.a->fail_read) atomicMin(c.a->fail_read, c.rd);
}

DEVINL uint8_t *slot_unit(K2Ctx &c, int s) { return c.sc + c.y.unit0 + (size_t)s * K2_SLOT_UNIT; }
DEVINL int *slot_score(K2Ctx &c, int s) { return (int *)(c.sc + c.y.score0) + (size_t)s * K2_SLOT_SCORE; }
// A unit slot is 1 KB of codes + 2 KB of node frequencies.  Copied word by word in a lane-strided loop, every word was a load the next store had to
// wait for (source and destination may alias as far as the compiler knows): 12 dependent memory round trips per copy.  All of a copy's loads first,
// then its stores: one round trip.
template <int NW>
DEVINL void wave_copy_words(uint32_t *dst, const uint32_t *src)
{   // NW * 64 32-bit words
    const int lane = lane_id();
    uint32_t v[NW];
#pragma unroll
    for (int q = 0; q < NW; q++) v[q] = src[q * 64 + lane];
#pragma unroll
    for (int q = 0; q < NW; q++) dst[q * 64 + lane] = v[q];
}
static_assert(K2_SLOT_UNIT == 4 * 4 * 64 && K2_SLOT_SCORE == 8 * 64, "slot copies: 4 + 8 words per lane");
DEVINL void slot_copy_raw(uint8_t *du, int *ds, const uint8_t *su, const int *ss)
{
    wave_copy_words<K2_SLOT_UNIT / 256>((uint32_t *)du, (const uint32_t *)su);
    wave_copy_words<K2_SLOT_SCORE / 64>((uint32_t *)ds, (const uint32_t *)ss);
}
// a candidate's unit (U codes) and node frequencies (U ints, -1 behind them: clear_rr) from its slot of a block into a unit slot
DEVINL void slot_load_candidate(uint8_t *ub, int *us, const uint8_t *su, const int *ss, int U)
{
    const int lane = lane_id();
    int sv[K2_SLOT_SCORE / 64]; int bv[K2_SLOT_SCORE / 64];
#pragma unroll
    for (int q = 0; q < K2_SLOT_SCORE / 64; q++) { const int t = q * 64 + lane; sv[q] = t < U ? ss[t] : -1; bv[q] = t < U ? (int)su[t] : 0; }
#pragma unroll
    for (int q = 0; q < K2_SLOT_SCORE / 64; q++) { const int t = q * 64 + lane; us[t] = sv[q]; if (t < U) ub[t] = (uint8_t)bv[q]; }
}
// the unit alone (the staged revisions: a candidate's node frequencies stay in its record, nothing between polish and the record's emission looks at them)
DEVINL void slot_copy_unit_raw(uint8_t *du, const uint8_t *su) { wave_copy_words<K2_SLOT_UNIT / 256>((uint32_t *)du, (const uint32_t *)su); }
DEVINL void slot_copy_unit(K2Ctx &c, int dst, int src)
{
    const unsigned long long t0 = clk();
    slot_copy_unit_raw(slot_unit(c, dst), slot_unit(c, src));
    wave_sync_mem();
    wc_time(c.wc, CYC_SLOT_COPY, t0);
}
DEVINL void slot_copy(K2Ctx &c, int dst, int src)
{
    const unsigned long long t0 = clk();
    slot_copy_raw(slot_unit(c, dst), slot_score(c, dst), slot_unit(c, src), slot_score(c, src));
    wave_sync_mem();
    wc_time(c.wc, CYC_SLOT_COPY, t0);
}

DEVINL void trace_ev(K2Ctx &c, int type, int a0, int a1, int a2, int a3, int a4, int a5, int a6, int a7,
                     int a8, int a9, int a10, int a11, int a12, int a13)
{
    if (c.a->trace_cap <= 0 || lane_id() != 0 || !((c.a->trace_mask >> type) & 1)) return;
    unsigned n = atomicAdd(c.a->trace_n, 1u);
    if (n >= (unsigned)c.a->trace_cap) return;
    int *e = c.a->trace + (size_t)n * 16;
    e[0] = type; e[1] = c.rd; e[2] = a0; e[3] = a1; e[4] = a2; e[5] = a3; e[6] = a4; e[7] = a5; e[8] = a6; e[9] = a7;
    e[10] = a8; e[11] = a9; e[12] = a10; e[13] = a11; e[14] = a12; e[15] = a13;
}
DEVINL bool trace_on(const K2Ctx &c, int type) { return c.a->trace_cap > 0 && ((c.a->trace_mask >> type) & 1); }
DEVINL int unit_hash(const uint8_t *u, int n)
{   // order-sensitive checksum of a unit, for the trace only (callers test trace_on() first: it is a serial loop)
    unsigned h = 2166136261u;
    for (int i = 0; i < n; i++) h = (h ^ (unsigned)u[i]) * 16777619u;
    return (int)(h & 0x7fffffffu);
}

// ---------------------------------------------------------------------------------------------------------
// k-mer multiset
// ---------------------------------------------------------------------------------------------------------
DEVINL unsigned tab_hash(int key) { return (unsigned)key * 2654435761u; }

// The table is organised in buckets of 4 slots (16 bytes = one ds_read_b128 / global_load_dwordx4): a key lives
// in the first bucket of its probe sequence (home bucket, then the following ones) that had a free slot when it
// was inserted, and the slots of a bucket fill in order.  A look-up therefore ends at the first bucket whose
// last slot is empty.  With <= 50 % load almost every look-up - hit or miss - is ONE 16-byte read; the first
// build's one-slot linear probing needed ~15 dependent reads for the slowest of 64 lanes.
typedef int v4i __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i lds_v4i;

// Three layouts, chosen per table so that a look-up is ONE LDS read whenever the reference's own regime allows it
// (a walk step is a chain of dependent look-ups; with the counts of wide windows in global memory a step took
// ~2500 cycles, 20 % of the kernel):
//   TAB_DIRECT  k <= 6: 4^k 16-bit counters indexed by the k-mer itself, no keys (what the reference does for
//               k <= count_maxKmer, consensus.c:138-164); any window of up to 65535 positions;
//   TAB_PACKED  k <= 10 (20 key bits) and windows up to K2_TAB_MAX_WIDTH: one word per slot, key | count << 20;
//   TAB_SPLIT   everything else: keys in LDS (or global for windows > K2_TAB_MAX_WIDTH), counts in LDS when the
//               table has <= 1024 slots, else in global scratch.
enum { TAB_DIRECT = 0, TAB_PACKED = 1, TAB_SPLIT = 2 };
#define K2_PACK_KEY_BITS 20
#define K2_PACK_KEY_MASK ((1 << K2_PACK_KEY_BITS) - 1)

DEVINL unsigned tab_bucket(const Tab &t, int key) { return (tab_hash(key) >> 9) & t.mask; }

// count of `key` (freq_node, consensus.c:229-253); any lane may ask for any key.  FMT = the table's layout.
template <int FMT>
DEVINL int tab_get_raw(lds_int *keys, const Tab &t, int key)
{
    if (FMT == TAB_DIRECT) {
        if ((unsigned)key >= t.nslots) return 0;
        const unsigned w = (unsigned)keys[key >> 1];
        return (int)((w >> (16 * (key & 1))) & 0xffffu);
    }
    unsigned b = tab_bucket(t, key);
    if (FMT == TAB_PACKED) {
        for (unsigned n = 0; n <= t.mask; n++) {
            const v4i kk = *(const lds_v4i *)(keys + 4 * b);
            // an empty slot is all ones: its count field (4095) cannot occur, so the key comparison alone would be
            // fooled only by the key of twenty 1-bits; compare the slot against "not empty" too
            int hit = -1;
            if ((kk.x & K2_PACK_KEY_MASK) == key && kk.x != K2_EMPTY) hit = kk.x;
            else if ((kk.y & K2_PACK_KEY_MASK) == key && kk.y != K2_EMPTY) hit = kk.y;
            else if ((kk.z & K2_PACK_KEY_MASK) == key && kk.z != K2_EMPTY) hit = kk.z;
            else if ((kk.w & K2_PACK_KEY_MASK) == key && kk.w != K2_EMPTY) hit = kk.w;
            if (hit != -1) return (int)((unsigned)hit >> K2_PACK_KEY_BITS);
            if (kk.w == K2_EMPTY) return 0;
            b = (b + 1) & t.mask;
        }
        return 0;
    }
    for (unsigned n = 0; n <= t.mask; n++) {
        v4i kk = t.use_lds ? *(const lds_v4i *)(keys + 4 * b) : *(const v4i *)(t.gkeys + 4 * b);
        int slot = kk.x == key ? 0 : kk.y == key ? 1 : kk.z == key ? 2 : kk.w == key ? 3 : -1;
        if (slot >= 0) return t.vals_lds ? keys[K2_VALS_LDS_OFF + 4 * b + slot] : t.gvals[4 * b + slot];
        if (kk.w == K2_EMPTY) return 0;
        b = (b + 1) & t.mask;
    }
    return 0;
}
// The first probe of tab_get_raw without a loop: the count if the key sits in its home bucket or the bucket has a free
// slot (the key is then absent); `more` = the bucket is full of other keys, or the table lies in global memory: ask
// tab_get_raw.  At the tables' load (<= 68 %) nearly every look-up ends here, and a walk's look-ups (five lanes of one walk,
// or four per lane in the seed screen) no longer pay a divergent loop each.
template <int FMT>
DEVINL int tab_get_first(lds_int *keys, const Tab &t, int key, bool &more)
{
    more = false;
    if (FMT == TAB_DIRECT) return tab_get_raw<TAB_DIRECT>(keys, t, key);
    if (FMT == TAB_SPLIT && !t.use_lds) { more = true; return 0; }
    const unsigned b = tab_bucket(t, key);
    const v4i kk = *(const lds_v4i *)(keys + 4 * b);
    if (FMT == TAB_PACKED) {
        int hit = -1;
        hit = ((kk.w & K2_PACK_KEY_MASK) == key && kk.w != K2_EMPTY) ? kk.w : hit;
        hit = ((kk.z & K2_PACK_KEY_MASK) == key && kk.z != K2_EMPTY) ? kk.z : hit;
        hit = ((kk.y & K2_PACK_KEY_MASK) == key && kk.y != K2_EMPTY) ? kk.y : hit;
        hit = ((kk.x & K2_PACK_KEY_MASK) == key && kk.x != K2_EMPTY) ? kk.x : hit;
        more = hit == -1 && kk.w != K2_EMPTY;
        return hit == -1 ? 0 : (int)((unsigned)hit >> K2_PACK_KEY_BITS);
    }
    const int slot = kk.x == key ? 0 : kk.y == key ? 1 : kk.z == key ? 2 : kk.w == key ? 3 : -1;
    more = slot < 0 && kk.w != K2_EMPTY;
    if (slot < 0) return 0;
    return t.vals_lds ? keys[K2_VALS_LDS_OFF + 4 * b + slot] : t.gvals[4 * b + slot];
}
DEVINL int tab_get(const K2Ctx &c, int key)
{
    if (c.tab.fmt == TAB_DIRECT) return tab_get_raw<TAB_DIRECT>(c.lds_keys, c.tab, key);
    if (c.tab.fmt == TAB_PACKED) return tab_get_raw<TAB_PACKED>(c.lds_keys, c.tab, key);
    return tab_get_raw<TAB_SPLIT>(c.lds_keys, c.tab, key);
}
// slot `sidx` of the table (sidx < nslots) for the look-ahead's table scans: key (K2_EMPTY if the slot holds none) and count
DEVINL void tab_slot(const K2Ctx &c, unsigned sidx, int &key, int &cnt)
{
    const Tab &t = c.tab;
    if (t.fmt == TAB_DIRECT) {
        const unsigned w = (unsigned)c.lds_keys[sidx >> 1];
        cnt = (int)((w >> (16 * (sidx & 1u))) & 0xffffu);
        key = cnt > 0 ? (int)sidx : K2_EMPTY;
    } else if (t.fmt == TAB_PACKED) {
        const int w = c.lds_keys[sidx];
        key = w == K2_EMPTY ? K2_EMPTY : (w & K2_PACK_KEY_MASK);
        cnt = (int)((unsigned)w >> K2_PACK_KEY_BITS);
    } else {
        key = t.use_lds ? c.lds_keys[sidx] : t.gkeys[sidx];
        cnt = key == K2_EMPTY ? 0 : (t.vals_lds ? c.lds_keys[K2_VALS_LDS_OFF + sidx] : t.gvals[sidx]);
    }
}
// decrement the count of a key known to be present (seed listing, consensus.c:160,209); one lane calls this
DEVINL void tab_dec(K2Ctx &c, int key)
{
    const Tab &t = c.tab;
    if (t.fmt == TAB_DIRECT) {
        (void)__hip_atomic_fetch_add(&c.lds_keys[key >> 1], -(1 << (16 * (key & 1))), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
    unsigned b = tab_bucket(t, key);
    for (unsigned n = 0; n <= t.mask; n++) {
        for (int sl = 0; sl < 4; sl++) {
            if (t.fmt == TAB_PACKED) {
                const int w = c.lds_keys[4 * b + sl];
                if (w != K2_EMPTY && (w & K2_PACK_KEY_MASK) == key) { c.lds_keys[4 * b + sl] = w - (1 << K2_PACK_KEY_BITS); return; }
            } else {
                int k = t.use_lds ? c.lds_keys[4 * b + sl] : t.gkeys[4 * b + sl];
                if (k == key) { if (t.vals_lds) c.lds_keys[K2_VALS_LDS_OFF + 4 * b + sl]--; else t.gvals[4 * b + sl]--; return; }
            }
        }
        b = (b + 1) & t.mask;
    }
}

// (node of window position i: win_node, walk_screen.h)

// build the table of window [qs,qe] for k; returns the maximum frequency (consensus.c:138-146/172-196)
DEVINL int tab_build(K2Ctx &c, int k, int qs, int qe)
{
    const int lane = lane_id();
    const int width = qe - qs + 1;
    const unsigned long long t0 = clk();
    Tab t;
    t.gkeys = (int *)(c.sc + c.y.gkeys); t.gvals = (int *)(c.sc + c.y.gvals);
    unsigned cap = 64; while (cap < 2u * (unsigned)width) cap <<= 1;          // slots; load <= 50 % (LDS: <= 68 %)
    t.use_lds = width <= K2_TAB_MAX_WIDTH;
    if (t.use_lds && cap > K2_TAB_CAP) cap = K2_TAB_CAP;
    t.mask = cap / 4 - 1;                                                      // buckets - 1
    t.vals_lds = t.use_lds && cap <= K2_VALS_LDS_OFF;
    t.nslots = cap;
    t.fmt = TAB_SPLIT;
    if (k <= 6 && width <= 65535) { t.fmt = TAB_DIRECT; t.nslots = 1u << (2 * k); t.use_lds = 1; t.vals_lds = 1; }
    else if (2 * k <= K2_PACK_KEY_BITS && t.use_lds) { t.fmt = TAB_PACKED; t.vals_lds = 1; }
    int mx = 0;
    if (t.fmt == TAB_DIRECT) {
        const unsigned words = t.nslots >= 2u ? t.nslots / 2u : 1u;
        for (unsigned s = lane; s < words; s += 64) c.lds_keys[s] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier();
    } else if (t.fmt == TAB_PACKED) {
        for (unsigned s = lane; s < cap; s += 64) c.lds_keys[s] = K2_EMPTY;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier();
    } else if (t.vals_lds) {
        for (unsigned s = lane; s < cap; s += 64) { c.lds_keys[s] = K2_EMPTY; c.lds_keys[K2_VALS_LDS_OFF + s] = 0; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier();
    } else if (t.use_lds) {
        for (unsigned s = lane; s < cap; s += 64) { c.lds_keys[s] = K2_EMPTY; t.gvals[s] = 0; }
        wave_sync_mem();
    } else {
        wc_add(c.wc, CNT_GLOBAL_TABLES, 1);
        for (unsigned s = lane; s < cap; s += 64) { t.gkeys[s] = K2_EMPTY; t.gvals[s] = 0; }
        wave_sync_mem();
    }
    if (t.fmt == TAB_SPLIT && !t.use_lds) {
        // A table in global memory (a window beyond K2_TAB_MAX_WIDTH: long reads): an insertion is a compare-and-swap that comes back from memory, one round trip
        // per probe - and per 64 window positions when the chunks take turns (a 40 000-position window: 625 round trips; 136 000 such tables per launch of 100 reads
        // of 42 kb, 45 G of its wavefront-cycles).  FOUR chunks' probes are in flight together here: same probe order per key (the slots of the home bucket, then
        // the next bucket's), same table whatever the interleaving (which of two new keys takes a slot first was never fixed).
        for (int base = qs; base <= qe; base += 256) {
            int key[4]; unsigned at[4]; bool live[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = base + 64 * u + lane;
                live[u] = i <= qe;
                key[u] = live[u] ? win_node(c.pk, c.L, k, qe, i) : 0;
                at[u] = 4u * tab_bucket(t, key[u]);
            }
            for (unsigned n = 0; n <= 4u * t.mask + 4u; n++) {
                if (__ballot(live[0] || live[1] || live[2] || live[3]) == 0ull) break;
                int prev[4];
#pragma unroll
                for (int u = 0; u < 4; u++) prev[u] = live[u] ? atomicCAS(&t.gkeys[at[u]], K2_EMPTY, key[u]) : 0;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (!live[u]) continue;
                    if (prev[u] == K2_EMPTY || prev[u] == key[u]) {
                        (void)__hip_atomic_fetch_add(&t.gvals[at[u]], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (the maximum is read off the counts below)
                        live[u] = false;
                    } else at[u] = (at[u] & 3u) == 3u ? 4u * (((at[u] >> 2) + 1u) & t.mask) : at[u] + 1u;
                }
                loop_join();
            }
            loop_join();
        }
    } else
    for (int base = qs; base <= qe; base += 64) {
        int i = base + lane;
        if (i <= qe) {
            int key = win_node(c.pk, c.L, k, qe, i);
            if (t.fmt == TAB_DIRECT) {
                const int sh = 16 * (key & 1);
                const unsigned old = (unsigned)__hip_atomic_fetch_add(&c.lds_keys[key >> 1], 1 << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const int nv = (int)((old >> sh) & 0xffffu) + 1;
                mx = nv > mx ? nv : mx;
            } else if (t.fmt == TAB_PACKED) {
                unsigned bk = tab_bucket(t, key);
                bool done = false;
                for (unsigned n = 0; n <= t.mask && !done; n++) {
                    for (int sl = 0; sl < 4 && !done; sl++) {
                        const unsigned at = 4 * bk + (unsigned)sl;
                        int expected = K2_EMPTY;
                        const bool won = __hip_atomic_compare_exchange_strong(&c.lds_keys[at], &expected, key | (1 << K2_PACK_KEY_BITS), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (won) { mx = mx > 1 ? mx : 1; done = true; }
                        else if ((expected & K2_PACK_KEY_MASK) == key) {     // `expected` holds the slot's word: never empty here
                            const unsigned old = (unsigned)__hip_atomic_fetch_add(&c.lds_keys[at], 1 << K2_PACK_KEY_BITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            const int nv = (int)(old >> K2_PACK_KEY_BITS) + 1;
                            mx = nv > mx ? nv : mx; done = true;
                        }
                    }
                    bk = (bk + 1) & t.mask;
                }
            } else {
                unsigned bk = tab_bucket(t, key);
                bool done = false;
                for (unsigned n = 0; n <= t.mask && !done; n++) {
                    for (int sl = 0; sl < 4 && !done; sl++) {
                        const unsigned at = 4 * bk + (unsigned)sl;
                        int seen;
                        if (t.use_lds) {
                            int expected = K2_EMPTY;
                            bool won = __hip_atomic_compare_exchange_strong(&c.lds_keys[at], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            seen = won ? key : expected;
                        } else {
                            int prev = atomicCAS(&t.gkeys[at], K2_EMPTY, key);
                            seen = prev == K2_EMPTY ? key : prev;
                        }
                        if (seen == key) {
                            if (t.vals_lds) {
                                const int nv = __hip_atomic_fetch_add(&c.lds_keys[K2_VALS_LDS_OFF + at], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + 1;
                                mx = nv > mx ? nv : mx;
                            } else {
                                // counts in global memory: the add does not come back (a returning atomic is a memory round trip in every one of the window's
                                // ~20 chunks - 64 000 such tables per launch at 85 000 cycles each); the maximum is read off the counts afterwards
                                (void)__hip_atomic_fetch_add(&t.gvals[at], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                            done = true;
                        }
                    }
                    bk = (bk + 1) & t.mask;
                }
            }
        }
    }
    wave_sync_mem();
    if (t.fmt == TAB_SPLIT && !t.vals_lds) {
        // (the slots' counts, eight loads in flight per lane)
        for (unsigned base = 0; base < cap; base += 512) {
            int v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) { const unsigned sidx = base + 64u * (unsigned)q + (unsigned)lane; v[q] = sidx < cap ? __hip_atomic_load(&t.gvals[sidx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0; }    // (where the atomics ran: L2)
#pragma unroll
            for (int q = 0; q < 8; q++) mx = v[q] > mx ? v[q] : mx;
        }
    }
    // A table in global memory has 2-4 slots per window position and the look-ahead's general steps SCAN it (every slot, once or
    // twice per step, hundreds of steps per failing walk: 5 M slots for one (window, k) of a 42 kb read, the longest work item of a
    // batch of such reads).  The distinct keys are listed once more, compact: the scans then touch a third to a tenth of the entries.
    t.n_compact = -1; t.ckeys = (int *)(c.sc + c.y.ckeys); t.cslots = (int *)(c.sc + c.y.cslots);
    if (!t.use_lds && t.fmt == TAB_SPLIT) {
        int nc = 0;
        for (unsigned base = 0; base < cap; base += 512) {                 // (eight loads in flight per lane: one memory round trip per 512 slots, not per 64)
            int kq[8];
#pragma unroll
            for (int q = 0; q < 8; q++) { const unsigned sidx = base + 64u * (unsigned)q + (unsigned)lane; kq[q] = sidx < cap ? t.gkeys[sidx] : K2_EMPTY; }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const unsigned sidx = base + 64u * (unsigned)q + (unsigned)lane;
                const int key = kq[q];
                const unsigned long long m = __ballot(key != K2_EMPTY);
                if (key != K2_EMPTY) { const int at = nc + mbcnt(m); t.ckeys[at] = key; t.cslots[at] = (int)sidx; }
                nc += __popcll(m);
            }
        }
        t.n_compact = nc;
        wave_sync_mem();
    }
    c.tab = t; c.tab_k = k;
    {   // The look-ahead decisions remembered for the previous table are void: an entry carries the number of the table it was written under,
        // and this table gets a new one.  (Before: the 256 entries of the small cache were cleared for every table - 2.5 M tables per launch of
        // 10 000 reads, 1 KB of strided stores each: a third of the walk kernels' HBM writes.)  What a wavefront must not meet is an entry of
        // an EARLIER kernel with a number it will hand out again: the region is cleared once per kernel and wavefront, on first use.  A table in
        // global memory (a window wider than K2_TAB_MAX_WIDTH) uses the whole cache: its failing walks take hundreds of general steps, which
        // the next seeds repeat
        c.tab_gen++;
        const int nsc = t.use_lds ? K2_STEP_CACHE_LDS : K2_STEP_CACHE;
        const int bit = t.use_lds ? 1 : 3;
        if ((c.sc_ready & bit) != bit) {
            int4 *sc_ = (int4 *)(c.sc + c.y.step_cache);
            for (int q = lane; q < 2 * nsc; q += 64) sc_[q] = make_int4(-1, 0, 0, 0);
            c.sc_ready |= bit;
            wave_sync_mem();
        }
    }
    wc_add(c.wc, CNT_TABLES, 1);
    mx = wave_max_i32_dpp(mx);                                                 // wave-uniform (readlane)
    wc_time(c.wc, CYC_TAB_BUILD, t0);
#ifdef MTR_PROFILE_WALK_FMT
    if (MTR_PROFILE_WALK_FMT >= 4) {   // development build: table builds by layout, every kernel - 4: cycles, 5: tables
        const int cls_ = t.fmt == TAB_DIRECT ? (k <= 4 ? CNT_SPARE43 : CNT_SPARE44) : t.fmt == TAB_PACKED ? (t.nslots <= 1024u ? CNT_SPARE45 : CNT_SPARE46)
                         : t.use_lds ? CNT_SPARE47 : CNT_SPARE55;
        if (MTR_PROFILE_WALK_FMT == 4) wc_time(c.wc, cls_, t0); else wc_add(c.wc, cls_, 1);
    }
#endif
    return mx;
}

// generate_freqNode_return_list_maxNodes' listing step (consensus.c:148-164/198-224): nodes whose count
// equals max_freq in first-occurrence order; each listed node's count is decremented; at most MAX_SEEDS.
DEVINL int tab_seeds(K2Ctx &c, int k, int qs, int qe, int max_freq)
{
    const int lane = lane_id();
    const unsigned long long t0 = clk();
    int n = 0;
    for (int base = qs; base <= qe && n < MTRC_MAX_SEEDS; base += 64) {
        int i = base + lane;
        int key = 0; bool cand = false;
        if (i <= qe) { key = win_node(c.pk, c.L, k, qe, i); cand = (tab_get(c, key) == max_freq); }
        unsigned long long m = __ballot(cand);
        while (m != 0ull && n < MTRC_MAX_SEEDS) {
            int t = first_lane(m);
            int sk = lane_val(key, t);
            if (lane == 0) { c.seeds[n] = sk; tab_dec(c, sk); }
            n++;
            m &= ~__ballot(cand && key == sk);      // later occurrences of the same node now see max_freq-1
            m &= ~(1ull << t);
            loop_join();
        }
        loop_join();
    }
    wave_sync_mem();
    wc_time(c.wc, CYC_SEEDS, t0);
    return n;
}

DEVINL unsigned rev_pairs(unsigned x)
{   // reverse the order of the 2-bit digits of a 32-bit word
    x = __brev(x);
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}

// ---------------------------------------------------------------------------------------------------------
// Look-ahead tie-breaking of one walk step (consensus.c:299-334 forward, :383-415 backward).
//
// Reference: level m = 1..look evaluates the 4*|T| candidates built from the tie list T of the previous level
// (scan order: tie-major, base-minor), keeps those whose count equals the maximum (first 1024 in scan order) as
// the next T, and stops when exactly one is left.  When a walk has strayed off the window's k-mers every
// candidate is absent, everything ties at count 0 and T quadruples per level up to the 1024 cap: ~5 500 table
// look-ups per step, for hundreds of steps - a handful of such walks made single reads 10x slower than the
// median and set the kernel's tail.  Same results, less work:
//   * T is kept COMPRESSED as (B, e): the first min(|B|*4^e, 1024) entries of B expanded e times in scan order.
//     B is the explicit list from the last level that had a present candidate ([0] initially).  An all-absent
//     level just increments e.  (Forward expansion appends free low digits; backward expansion prepends them in
//     reversed significance - the reference's msd-first enumeration.)
//   * a level with many candidates is evaluated by SCANNING THE TABLE instead of probing it: a key is a
//     candidate iff its fixed part matches the node (top k-m digits forward, low k-m digits backward) and its
//     digit string decomposes into (b in B, free digits within the cap, last base); absent candidates have count
//     0 by definition.  The few present ones are ranked by their scan index to form the next explicit list.
// Returns the reference's max_lsd / max_msd (first candidate with the final maximum); m_exit = its loop variable.
// ---------------------------------------------------------------------------------------------------------
DEVINL unsigned rev_digits(unsigned x, int e)
{   // reverse the order of the low e base-4 digits of x
    if (e <= 0) return 0u;
    unsigned r = __brev(x);
    r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
    return r >> (32 - 2 * e);
}

// ---- the keys of a table in global memory, grouped (round 5) ------------------------------------------------------------------------------------
// A general look-ahead step scans the table's compact key list (once to find the first level that has a candidate at a dead end, once for that level's
// candidates): 16 000 keys for a 16 kb window of a 42 kb read, hundreds of such steps in a failing walk - 14 ms for ONE (window, k), the longest work item of a
// launch of such reads.  The candidates of a level share their fixed part: the node's last k - m digits as the key's FIRST digits (forward), its first k - m
// as the key's LAST digits (backward).  One counting sort groups the keys by their first five digits (backward: by their last five, the bucket number with
// its digits reversed, so that a shorter fixed part is still a contiguous stretch of buckets); the bucket ends stay in LDS, which a table in global memory
// leaves idle (1 024 words per direction).  A level's candidates are then the entries of one bucket - or of 4^(5 - f) neighbouring ones when the fixed part
// has f < 5 digits - and the scans run over those: a few chunks instead of hundreds.  Made when a table's first general step in a direction needs it.
#define K2_IDX_MIN_KEYS 512        // fewer keys than this: the scans of the whole list are a few chunks anyway
DEVINL unsigned idx_bucket(bool backward, unsigned key, int k)
{
    return backward ? rev_digits(key & 1023u, 5) : (key >> (2 * k - 10));
}
DEVINL void idx_build(K2Ctx &c, bool backward, int k)
{
    const int lane = lane_id();
    const Tab &t = c.tab;
    const int n = t.n_compact;
    lds_int *ends = c.lds_keys + (backward ? 1024 : 0);
    int *gk = (int *)(c.sc + (backward ? c.y.gkb : c.y.gkf)), *gs = (int *)(c.sc + (backward ? c.y.gsb : c.y.gsf));
    for (int b = lane; b < 1024; b += 64) ends[b] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier();
    for (int base = 0; base < n; base += 512) {                       // bucket sizes (eight loads in flight per lane)
        int kq[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { const int i = base + 64 * q + lane; kq[q] = i < n ? t.ckeys[i] : K2_EMPTY; }
#pragma unroll
        for (int q = 0; q < 8; q++) if (kq[q] != K2_EMPTY) (void)__hip_atomic_fetch_add(&ends[idx_bucket(backward, (unsigned)kq[q], k)], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
    {   // exclusive prefix sums: lane l owns buckets 16 l .. 16 l + 15
        int cnt[16], sum = 0;
#pragma unroll
        for (int q = 0; q < 16; q++) { cnt[q] = ends[16 * lane + q]; sum += cnt[q]; }
        int incl = sum;
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
        int run = incl - sum;
#pragma unroll
        for (int q = 0; q < 16; q++) { ends[16 * lane + q] = run; run += cnt[q]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
    for (int base = 0; base < n; base += 512) {                       // every entry to its bucket: the bucket's start moves up to its end
        int kq[8], sq[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { const int i = base + 64 * q + lane; kq[q] = i < n ? t.ckeys[i] : K2_EMPTY; sq[q] = i < n ? t.cslots[i] : 0; }
#pragma unroll
        for (int q = 0; q < 8; q++) if (kq[q] != K2_EMPTY) {
            const int at = __hip_atomic_fetch_add(&ends[idx_bucket(backward, (unsigned)kq[q], k)], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            gk[at] = kq[q]; gs[at] = sq[q];
        }
    }
    wave_sync_mem();
    if (backward) c.idx_gen_b = c.tab_gen; else c.idx_gen_f = c.tab_gen;
}
// the entries [lo, hi) of the grouped list that hold every key whose fixed part (f digits: `fixed`) is the one asked for
DEVINL void idx_range(const K2Ctx &c, bool backward, unsigned fixed, int f, int &lo, int &hi)
{
    const lds_int *ends = c.lds_keys + (backward ? 1024 : 0);
    unsigned blo, bhi;
    if (f >= 5) { blo = backward ? rev_digits(fixed & 1023u, 5) : (fixed >> (2 * (f - 5))); bhi = blo; }
    else {
        const unsigned r = backward ? rev_digits(fixed, f) : fixed;    // (f = 0: every bucket)
        blo = r << (2 * (5 - f)); bhi = ((r + 1u) << (2 * (5 - f))) - 1u;
    }
    lo = blo == 0u ? 0 : uni(ends[blo - 1u]);
    hi = uni(ends[bhi]);
}

DEVINL int lookahead(K2Ctx &c, bool backward, int node, int k, int look, int &m_exit, long long &lookups)
{
    const int lane = lane_id();
    const Tab &t = c.tab;
    const unsigned cap = t.nslots;
    {   // Level 1 = the four successors of the node (all that most steps ever need): lanes 0..3 probe the table, the
        // comparison runs on the scalar unit.  A unique maximum (or look == 1) ends the step here; a tie with more
        // levels to go falls into the general loop below, which starts again at level 1.
        const int s1 = k - 1;
        int cnt1 = -1;
        if (lane < 4) {
            const int cand = !backward ? (((node & ((1 << (2 * s1)) - 1)) << 2) + lane) : ((lane << (2 * s1)) + (node >> 2));
            cnt1 = tab_get(c, cand);
        }
        const int c0 = lane_val(cnt1, 0), c1 = lane_val(cnt1, 1), c2 = lane_val(cnt1, 2), c3 = lane_val(cnt1, 3);
        int bst = c0, first = 0;
        if (c1 > bst) { bst = c1; first = 1; }
        if (c2 > bst) { bst = c2; first = 2; }
        if (c3 > bst) { bst = c3; first = 3; }
        const int nf1 = (c0 == bst ? 1 : 0) + (c1 == bst ? 1 : 0) + (c2 == bst ? 1 : 0) + (c3 == bst ? 1 : 0);
        wc_add(c.wc, CNT_WALK_STEPS, 1);
        if (nf1 == 1 || look == 1) { lookups += 4; m_exit = nf1 == 1 ? 1 : 2; return first; }
    }
    wc_add(c.wc, CNT_WALK_SLOW, 1);
    const unsigned long long t_slow = clk();
    // a table in global memory with enough keys: its scans run over the entries that share the level's fixed part (idx_build above)
    const bool grouped = t.n_compact >= K2_IDX_MIN_KEYS && k >= 5;
    if (grouped && (backward ? c.idx_gen_b : c.idx_gen_f) != c.tab_gen) idx_build(c, backward, k);
    const int *gk = (const int *)(c.sc + (backward ? c.y.gkb : c.y.gkf)), *gs = (const int *)(c.sc + (backward ? c.y.gsb : c.y.gsf));
    int *B = c.ties, *Bn = c.fresh;
    int nb = 1, e = 0, m0 = 0;
    int breg = 0;                                   // lane i holds B[i] (i < min(nb,64))
    int best_digit = 0;
    int m;
    for (m = 1; m <= look; m++) {                   // invariant: m == m0 + e + 1
        const int nt = (e >= 5 || (nb << (2 * e)) >= MTRC_MAX_TIEBREAKS) ? MTRC_MAX_TIEBREAKS : (nb << (2 * e));
        const int ncand = 4 * nt;
        const int s = k - m;
        const int fixed = backward ? (node >> (2 * m)) : (node & ((1 << (2 * s)) - 1));
        const int emask = (1 << (2 * e)) - 1;
        int best = -1, nf = 0;
        best_digit = 0;
        bool evaluated = false;
        if (m == 2 && m0 == 0 && e == 1 && look > 2) {
            // Dead end at level 1 (all four successors absent): the list is the complete one and stays complete
            // while levels are all-absent.  ONE scan of the table finds the first level that has a present
            // candidate; the levels before it are all-absent by definition and are skipped.
            const int top = look < 12 ? look : 12;
            // per level mm (2..top): a key is a candidate iff its fixed part equals the node's ((key ^ shifted node) & fixed-part mask == 0) and its free digits
            // stay inside the 1024 cap (digits beyond the first five free ones are 0).  Both are ONE unsigned comparison per level:
            //   forward   fixed part on top, free digits below:  (key ^ ((node << 2mm) mod 4^k)) < 4^min(mm, 6)
            //   backward  fixed part at the bottom, the digits that must be 0 right above it: the bit-reversed key has them on top -
            //             (rev(key) ^ rev(node >> 2mm)) <= 2^(32 - w) - 1,  w = 2 (k - mm) + 2 max(0, mm - 6) bits that must agree
            // (round 1 formed two masks, an AND, an OR and a compare + select per level: ~7 vector instructions; three now, the hit bits collected by add-with-carry)
            unsigned hits = 0u;                                             // bit mm - 2 = this lane saw a candidate of level mm
            const unsigned kmask = (k >= 16) ? 0xffffffffu : ((1u << (2 * k)) - 1u);
            unsigned lvN[11], lvT[11];
#pragma unroll
            for (int mm = 2; mm <= 12; mm++) {
                const int wbits = 2 * (k - mm) + (mm > 6 ? 2 * (mm - 6) : 0);
                if (!backward) { lvN[mm - 2] = ((unsigned)node << (2 * (mm < 16 ? mm : 15))) & kmask; lvT[mm - 2] = (1u << (mm < 6 ? 2 * mm : 12)) - 1u; }
                else { lvN[mm - 2] = mm <= top ? __builtin_bitreverse32((unsigned)node >> (2 * mm)) : 0u; lvT[mm - 2] = (mm > top || wbits <= 0) ? 0xffffffffu : ((1u << (32 - wbits)) - 1u); }
            }
            const bool compact = t.n_compact >= 0;
            const unsigned nscan = compact ? (unsigned)t.n_compact : cap;
            if (grouped) {
                // level by level, lowest first: the entries that share the level's fixed part (a bucket or a stretch of buckets), the same comparison
                for (int mm = 2; mm <= top && hits == 0u; mm++) {
                    const int f = k - mm;
                    const unsigned fx = backward ? ((unsigned)node >> (2 * mm)) : ((unsigned)node & ((1u << (2 * f)) - 1u));
                    int lo, hi;
                    idx_range(c, backward, fx, f, lo, hi);
                    const int wb = 2 * f + (mm > 6 ? 2 * (mm - 6) : 0);     // (the level's comparison, as in the table of levels above)
                    const unsigned gN = !backward ? (((unsigned)node << (2 * mm)) & kmask) : __builtin_bitreverse32((unsigned)node >> (2 * mm));
                    const unsigned gT = !backward ? ((1u << (mm < 6 ? 2 * mm : 12)) - 1u) : (wb <= 0 ? 0xffffffffu : ((1u << (32 - wb)) - 1u));
                    for (int base = lo; base < hi; base += 64) {
                        const int i = base + lane;
                        const int keyi = i < hi ? gk[i] : K2_EMPTY;
                        const unsigned x = backward ? __builtin_bitreverse32((unsigned)keyi) : (unsigned)keyi;
                        if (__ballot(keyi != K2_EMPTY && (x ^ gN) <= gT) != 0ull) { hits = 1u << (mm - 2); break; }
                    }
                    lookups += hi - lo;
                }
            } else
            for (unsigned base = 0; base < nscan; base += 64) {
                const unsigned sidx = base + (unsigned)lane;
                int keyi = K2_EMPTY, cnti = 0;
                if (sidx < nscan) { if (compact) keyi = t.ckeys[sidx]; else tab_slot(c, sidx, keyi, cnti); }
                const unsigned x = backward ? __builtin_bitreverse32((unsigned)keyi) : (unsigned)keyi;
                unsigned h = 0u, tmp;
#pragma unroll
                for (int mm = 12; mm >= 2; mm--)                            // (levels beyond `top` are masked out below)
                    asm("v_xor_b32 %1, %2, %3\n\tv_cmp_ge_u32 vcc, %4, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(h), "=&v"(tmp) : "s"(lvN[mm - 2]), "v"(x), "s"(lvT[mm - 2]) : "vcc");
                if (keyi != K2_EMPTY) hits |= h;
            }
            hits &= (1u << (top - 1)) - 1u;                                 // levels 2 .. top
            int first_hit = top + 1;
            for (int mm = top; mm >= 2; mm--) if (__ballot((hits >> (mm - 2)) & 1u) != 0ull) first_hit = mm;
            if (!grouped) lookups += nscan;
            if (first_hit > 2) {
                if (first_hit > look) {                                      // nothing present up to the last level
                    m = look + 1; best_digit = 0;
                    break;
                }
                e = first_hit - 1; m = first_hit - 1;                       // levels 2 .. first_hit-1 are all-absent
                continue;
            }
        }
        if (nb <= 64 && ncand >= 128 && (unsigned)ncand * 4u > (t.n_compact >= 0 ? (unsigned)t.n_compact : cap)) {
            // ---- scan the table ------------------------------------------------------------------------------
            int nmatch = 0;
            const bool compact = t.n_compact >= 0;
            unsigned nscan = compact ? (unsigned)t.n_compact : cap, scan0 = 0u;
            const int *sk = t.ckeys, *ss = t.cslots;
            if (grouped) {                                                  // only the entries that share the level's fixed part
                int lo, hi;
                idx_range(c, backward, (unsigned)fixed, s, lo, hi);
                scan0 = (unsigned)lo; nscan = (unsigned)hi; sk = gk; ss = gs;
            }
            for (unsigned base = scan0; base < nscan; base += 64) {
                const unsigned sidx = base + (unsigned)lane;
                int key = K2_EMPTY, scnt = 0;
                if (sidx < nscan) { if (compact) key = sk[sidx]; else tab_slot(c, sidx, key, scnt); }
                bool hit = key != K2_EMPTY;
                int d = 0;
                if (!backward) { hit = hit && ((key >> (2 * m)) == fixed); d = key & ((1 << (2 * m)) - 1); }
                else { hit = hit && ((key & ((1 << (2 * s)) - 1)) == fixed); d = (int)((unsigned)key >> (2 * s)); }
                int b, x, j;
                if (!backward) { j = d & 3; x = (d >> 2) & emask; b = d >> (2 * (e + 1)); }
                else { b = d & ((1 << (2 * m0)) - 1); j = d >> (2 * (m0 + e)); x = (int)rev_digits((unsigned)((d >> (2 * m0)) & emask), e); }
                int bi = -1;
                for (int q = 0; q < nb; q++) { const int bv = lane_val(breg, q); if (bv == b) bi = q; }
                const long long ti = bi < 0 ? -1 : (((long long)bi) << (2 * e)) + x;
                hit = hit && bi >= 0 && ti < MTRC_MAX_TIEBREAKS;
                const int idx = (int)ti * 4 + j;
                if (compact && hit) scnt = t.gvals[ss[sidx]];            // (the count of a listed key: only the few candidates look it up)
                const int cnt = hit ? scnt : -1;
                const unsigned long long hm = __ballot(hit);
                if (hm != 0ull) {
                    const int pos = nmatch + mbcnt(hm);
                    if (hit && pos < 64) { c.stage[pos] = cnt; c.stage[64 + pos] = idx; c.stage[128 + pos] = d; }
                    nmatch += __popcll(hm);
                }
                loop_join();
            }
            lookups += nscan - scan0;
            if (nmatch <= 64) {
                evaluated = true;
                if (nmatch == 0) {                                          // every candidate absent: all tie at 0
                    best = 0; nf = ncand < MTRC_MAX_TIEBREAKS ? ncand : MTRC_MAX_TIEBREAKS;
                    const int b0 = lane_val(breg, 0);
                    best_digit = backward ? b0 : (b0 << (2 * (e + 1)));
                } else {
                    __builtin_amdgcn_wave_barrier();
                    const bool mine = lane < nmatch;
                    const int cnt = mine ? c.stage[lane] : -1, idx = mine ? c.stage[64 + lane] : 0x7fffffff, d = mine ? c.stage[128 + lane] : 0;
                    best = wave_max_i32_dpp(cnt);
                    const bool tie = mine && cnt == best;
                    int rank = 0;
                    for (int q = 0; q < nmatch; q++) {
                        const int iq = lane_val(idx, q), cq = lane_val(cnt, q);
                        if (cq == best && iq < idx) rank++;
                    }
                    const unsigned long long tm = __ballot(tie);
                    nf = __popcll(tm);
                    if (tie) c.stage[192 + rank] = d;                       // <= 64 entries: the new list stays on chip
                    __builtin_amdgcn_wave_barrier();
                    best_digit = uni(c.stage[192]);
                }
            }
        }
        if (!evaluated) {
            // ---- probe every candidate -----------------------------------------------------------------------
            best = -1; nf = 0; best_digit = 0;
            const int p4m1 = 1 << (2 * (m - 1));
            for (int base = 0; base < ncand; base += 64) {
                const int ci = base + lane;
                int cnt = -1, digit = 0;
                const int ti = ci >> 2, j = ci & 3, bi = ti >> (2 * e), x = ti & emask;
                // the shuffle runs with all lanes active (a lane reading an inactive lane would get 0)
                const int bshfl = __shfl(breg, bi & 63, 64);
                if (ci < ncand) {
                    const int bval = (m0 == 0) ? 0 : (nb <= 64 ? bshfl : B[bi]);
                    int cand;
                    if (!backward) { const int tv = (bval << (2 * e)) | x; digit = 4 * tv + j; cand = ((node & ((1 << (2 * s)) - 1)) << (2 * m)) + digit; }   // :311-312
                    else { const int tv = bval + (int)(rev_digits((unsigned)x, e) << (2 * m0)); digit = j * p4m1 + tv; cand = (digit << (2 * s)) + (node >> (2 * m)); }   // :392-393
                    cnt = tab_get(c, cand);
                }
                const int cm = wave_max_i32_dpp(cnt);
                if (cm > best) { best = cm; nf = 0; }                        // a new maximum empties the list
                const unsigned long long eq = __ballot(ci < ncand && cnt == best);
                if (eq != 0ull) {
                    if (nf == 0) best_digit = lane_val(digit, first_lane(eq));
                    const int pos = nf + mbcnt(eq);
                    if (cnt == best && ci < ncand && pos < MTRC_MAX_TIEBREAKS) { if (pos < 64) c.stage[192 + pos] = digit; else Bn[pos] = digit; }
                    nf += __popcll(eq); if (nf > MTRC_MAX_TIEBREAKS) nf = MTRC_MAX_TIEBREAKS;
                }
                loop_join();
            }
            lookups += ncand;
        }
        if (nf <= 1) break;
        if (best == 0) {
            e += 1;                                                          // all absent: the list just expands
        } else {
            // the first 64 entries of the new list are in LDS (stage[192..]); longer lists (rare) continue in the
            // global tie arrays, where the first 64 are copied too
            __builtin_amdgcn_wave_barrier();
            nb = nf; e = 0; m0 = m;
            breg = lane < nb ? c.stage[192 + lane] : 0;
            if (nb > 64) { Bn[lane] = breg; wave_sync_mem(); int *sw = B; B = Bn; Bn = sw; }
        }
        loop_join();
    }
    m_exit = m;
    wc_time(c.wc, CYC_WALK_SLOW, t_slow);
    return best_digit;
}

// ---------------------------------------------------------------------------------------------------------
// greedy walks on the De Bruijn graph (consensus.c:269-505).  Writes bases/scores into slot `dst`.
// ---------------------------------------------------------------------------------------------------------
// The steps of a walk whose level-1 look-ahead decides (a unique best successor, or l < 10 where only one level is
// looked at: 91 % of all steps) run in an out-of-line function that has nothing but the walk in its registers: inlined
// into the per-read kernel the same loop spent most of its ~350 instructions per step reloading spilled scalars and
// branching over table layouts.  It returns BEFORE a step that needs the deeper look-ahead; walk() does that one
// step with lookahead() and calls it again.
// Cycle check (Brent): from step 10 on every step looks k levels ahead, so the next node is a function of the node
// alone.  A node that repeats there (the seed would have ended the walk) means the walk runs round a cycle that does not
// contain the seed until max_steps - the reference's answer is "no unit" (consensus.c:437-446), which is returned at
// once.  Walks that stray off the window's k-mers end in the all-A node, whose every step is a dead-end scan of the
// whole table: 43 % of the walk time before this check.
struct WalkState { int node, l, pend, pend_at, status, fast_steps, chk_node, chk_l, chk_pow; };
enum { WALK_RUNNING = 0, WALK_CLOSED = 1, WALK_CYCLE = 2 };
DEVINL bool walk_cycle_check(int node, int l, int &chk_node, int &chk_l, int &chk_pow)
{   // call after the step at index l >= 10 produced `node`; a walk starts with chk_node = -1 (no node), chk_l = -1, chk_pow = 1: the first call records
    if (node == chk_node) return true;
    if (l - chk_l >= chk_pow) { chk_node = node; chk_l = l; chk_pow *= 2; }
    return false;
}

typedef __attribute__((address_space(1))) uint8_t glb_u8;     // global_* stores (a flat store would also count in lgkmcnt and
typedef __attribute__((address_space(1))) int glb_int;        // hold up the next LDS read's wait)
// TWO steps per table round trip (round 5; tables in LDS with one read per look-up: TAB_DIRECT, TAB_PACKED).  The next node is always one of the four
// successors the step looks up, so THEIR successors can be looked up in the same instruction stream by lanes that would idle: lanes 0-3 hold the
// successors S_j of the node, lanes 4+4j .. 7+4j the successors of S_j, lane 20 (forward) the node itself.  One key computation, one hash, one ds_read,
// one pair of quad permutes and one ballot then decide two steps - what is left per step is scalar: which lanes of ITS quad hold the maximum, the node
// update, the two tests that end a walk.  A step was ~110 instructions (1 600 cycles with four wavefronts a SIMD on 2 048-slot tables, 10 M of a launch's 19 M
// steps); the look-ups were ~50 of them.  The unit's bases and node counts are collected in two registers (v_writelane at lane l mod 64) and stored 64 at a
// time instead of two single-lane stores a step.  Decisions, break conditions and stored values are those of the one-step-per-look-up loop this replaced (consensus.c:305-312 / :386-393), step for step.
// EARLY: the steps l < 10 (max_steps = at most 10: a tie takes the first of the tied successors - forward: base 0 -, nothing is checked for cycles); else the
// steps from 10 on (a tie ends the call, the cycle check runs) - two instances, so that neither tests l against 10 in its loop.
#define TAB_SPLIT_GLOBAL 3      // (walk_pair_steps only: TAB_SPLIT with the keys in global memory)
template <int FMT, bool BACKWARD, bool EARLY>
DEVINL void walk_pair_steps(lds_int *keys, const Tab &t, uint8_t *ub_, int *us_, int k, int seed, int max_steps, WalkState &w)
{
    // (TAB_SPLIT: only with the keys in LDS)
    const int lane = lane_id();
    glb_u8 *ub = (glb_u8 *)ub_; glb_int *us = (glb_int *)us_;
    const int sh1 = 2 * (k - 1), p4k1 = 1 << sh1, m1 = p4k1 - 1;
    const unsigned kmask = (1u << (2 * k)) - 1u;                                  // k <= 15
    // what a lane looks up: key = (node >> l_sh) + l_add (backward), ((node << l_sh) & kmask) + l_add (forward)
    const int q = lane - 4, jj = (q >> 2) & 3, cc = q & 3;
    const bool lvl1 = lane < 4, lvl2 = lane >= 4 && lane < 20;
    const bool active = lane < (BACKWARD ? 20 : 21);
    const int l_sh = lvl1 ? 2 : lvl2 ? 4 : 0;
    const int l_add = BACKWARD ? (lvl1 ? (lane << sh1) : lvl2 ? ((cc << sh1) + (jj << (sh1 - 2))) : 0)          // S_j = j 4^(k-1) + node / 4; its successor c: c 4^(k-1) + S_j / 4
                               : (lvl1 ? lane : lvl2 ? ((jj << 2) + cc) : 0);                                   // S_j = 4 (node mod 4^(k-1)) + j; its successor c: 4 (S_j mod 4^(k-1)) + c
    int node = w.node, l = w.l, pend = w.pend, status = WALK_RUNNING;
    const int l_in = l;
    int chk_node = w.chk_node, chk_l = w.chk_l, chk_pow = w.chk_pow;
    int lo = l, ubuf = 0, sbuf = 0;                       // lane i of ubuf / sbuf: ub[64 b + i] / us[64 b + i - 1] of the block b the walk is in; valid from lo on
    auto flush = [&](int hi) {
        const int li = (lo & ~63) + lane;
        if (li >= lo && li < hi) { ub[li] = (uint8_t)ubuf; if (li > 0) us[li - 1] = sbuf; }
    };
    // The scalar unit is what the walk kernels wait for (one SALU instruction per SIMD every four cycles, four wavefronts a SIMD, VALU idle): the
    // part of a step that is not look-ups is written with single exits (goto) and without flags the compiler would keep as 64-bit masks.
    int done = 0;                                         // steps performed past w.l, at the exit
    while (l < max_steps) {
        const unsigned key = BACKWARD ? ((unsigned)node >> l_sh) + (unsigned)l_add : ((((unsigned)node << l_sh) & kmask) + (unsigned)l_add);
        int cnt = -1;
        bool more = false;
        if (FMT == TAB_DIRECT) {
            const unsigned wd = (unsigned)keys[key >> 1];
            const int cv = (int)((wd >> (16 * (key & 1u))) & 0xffffu);
            cnt = active ? (key < t.nslots ? cv : 0) : -1;
        } else if (FMT == TAB_PACKED) {
            // The home bucket and the one after it, read side by side: a key sits in the first bucket of its probe sequence that had a free slot when it came, so
            // it can only be in the second if the first is full - the minimum below may run over all eight slots.  One bucket decided 89 % of the look-ups of
            // a 2 048-slot table (a ninth of its buckets are full), which left nine of ten step pairs - twenty look-ups each - with a lane in the probe loop.
            const unsigned b0 = (tab_hash((int)key) >> 9) & t.mask, b1 = (b0 + 1u) & t.mask;
            const v4i ka = *(const lds_v4i *)(keys + 4 * b0), kb = *(const lds_v4i *)(keys + 4 * b1);
            // slot ^ key, rotated so that the key bits are on top: a slot that holds the key is then its count (< 4 095), every other slot - other keys, the
            // empty slot (all ones: 4 095 in the count field) - is at least 4 095
            auto rot = [&](int wv) { const unsigned d = (unsigned)wv ^ key; return (unsigned)__builtin_amdgcn_alignbit(d, d, K2_PACK_KEY_BITS); };
            auto min3u = [](unsigned x, unsigned y, unsigned z) { const unsigned m = x < y ? x : y; return m < z ? m : z; };
            const unsigned mn = min3u(min3u(rot(ka.x), rot(ka.y), rot(ka.z)), min3u(rot(ka.w), rot(kb.x), rot(kb.y)), min3u(rot(kb.z), rot(kb.w), 0xffffffffu));
            const bool present = mn < 4095u;
            more = active && !present && ka.w != K2_EMPTY && kb.w != K2_EMPTY;              // both full of other keys: the key may sit further on
            cnt = active ? (present ? (int)mn : 0) : -1;
        }
        if (FMT == TAB_SPLIT || FMT == TAB_SPLIT_GLOBAL) {
            // keys in LDS, counts in LDS or - the 2 048-slot tables of k >= 11 - in global scratch: the same two buckets, the slot that holds the key, and
            // the count only for the keys that are there (one memory round trip for two steps).  A table in global memory (long reads): the same with its
            // keys from memory - two round trips for two steps instead of four
            const unsigned b0 = tab_bucket(t, (int)key), b1 = (b0 + 1u) & t.mask;
            v4i ka, kb;
            if (FMT == TAB_SPLIT) { ka = *(const lds_v4i *)(keys + 4 * b0); kb = *(const lds_v4i *)(keys + 4 * b1); }
            else if (active) { ka = *(const v4i *)(t.gkeys + 4 * b0); kb = *(const v4i *)(t.gkeys + 4 * b1); }
            else { ka = kb = (v4i){ K2_EMPTY, K2_EMPTY, K2_EMPTY, K2_EMPTY }; }
            const int ik = (int)key;
            int idx = kb.w == ik ? (int)(4u * b1 + 3u) : -1;
            idx = kb.z == ik ? (int)(4u * b1 + 2u) : idx; idx = kb.y == ik ? (int)(4u * b1 + 1u) : idx; idx = kb.x == ik ? (int)(4u * b1) : idx;
            idx = ka.w == ik ? (int)(4u * b0 + 3u) : idx; idx = ka.z == ik ? (int)(4u * b0 + 2u) : idx;
            idx = ka.y == ik ? (int)(4u * b0 + 1u) : idx; idx = ka.x == ik ? (int)(4u * b0) : idx;
            const bool present = active && idx >= 0;
            more = active && idx < 0 && ka.w != K2_EMPTY && kb.w != K2_EMPTY;
            int cv = 0;
            if (present) cv = (FMT == TAB_SPLIT && t.vals_lds) ? keys[K2_VALS_LDS_OFF + idx] : t.gvals[idx];
            cnt = active ? cv : -1;
        }
        // a lane whose look-up is not decided yet (rare) asks tab_get_raw - but only where its count is needed: the node's successors (and the node) now, the
        // successors of the chosen successor after the first step
        const unsigned more_m = FMT != TAB_DIRECT ? (unsigned)__ballot(more) : 0u;
        if (FMT != TAB_DIRECT && (more_m & (BACKWARD ? 0xfu : 0x10000fu)) != 0u) {
            if (more && (lane < 4 || lane == 20)) cnt = tab_get_raw<(FMT == TAB_SPLIT_GLOBAL ? TAB_SPLIT : FMT)>(keys, t, (int)key);
        }
        int qmax; unsigned eqm;
        auto quad_max = [&]() {
            int qm = __builtin_amdgcn_update_dpp(cnt, cnt, 0xB1, 0xf, 0xf, false);         // quad_perm [1,0,3,2]
            qm = qm > cnt ? qm : cnt;
            const int qm2 = __builtin_amdgcn_update_dpp(qm, qm, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
            qmax = qm2 > qm ? qm2 : qm;
            eqm = (unsigned)__ballot(cnt == qmax);                                         // bit: the lane holds its quad's maximum
        };
        quad_max();
        int base_lane = 0, self_lane = 20;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            if (FMT != TAB_DIRECT && half == 1 && ((more_m >> base_lane) & 0xfu) != 0u) {
                if (more && (lane >> 2) == (base_lane >> 2)) cnt = tab_get_raw<(FMT == TAB_SPLIT_GLOBAL ? TAB_SPLIT : FMT)>(keys, t, (int)key);
                quad_max();
            }
            const unsigned eq = (eqm >> base_lane) & 0xfu;                                 // never 0: some lane holds the maximum
            int dig = (int)__builtin_ctz(eq);
            if (eq & (eq - 1u)) {                                                          // a tie
                if (!EARLY) goto out;                                                      // more levels to look at: the general path decides
                if (!BACKWARD) dig = 0;                                                    // one level (l < 10): the loop variable ran out, base 0 (SURVEY H6)
            }
            const int prev = pend;                                                         // us[l - 1] (not stored for l = 0)
            if (!BACKWARD) {
                pend = lane_val(cnt, self_lane);
                write_lane2(sbuf, ubuf, prev, node >> sh1, l);
                node = 4 * (node & m1) + dig;
            } else {
                pend = lane_val(qmax, base_lane);
                node = dig * p4k1 + (node >> 2);
                write_lane2(sbuf, ubuf, prev, dig, l);
            }
            if (node == seed) { status = WALK_CLOSED; done = 1; goto out; }
            if (!EARLY) {
                if (node == chk_node) { status = WALK_CYCLE; done = 1; goto out; }
                if (l - chk_l >= chk_pow) { chk_node = node; chk_l = l; chk_pow *= 2; }
            }
            l++;
            if ((l & 63) == 0) { flush(l); lo = l; }
            if (l >= max_steps) goto out;
            self_lane = dig; base_lane = 4 + 4 * dig;                                      // the new node is S_dig: its count sits in lane dig, its successors in quad 1 + dig
        }
    }
out:
    flush(l + done);
    w.node = node; w.l = l; w.pend = pend; w.status = status; w.fast_steps = l + done - l_in;
    if (w.fast_steps > 0) w.pend_at = l + done - 1;
    w.chk_node = chk_node; w.chk_l = chk_l; w.chk_pow = chk_pow;
}

// Out of line, with nothing but the walk in its registers.  Everything travels in registers: a WalkState passed by pointer went through scratch memory - two round
// trips inside the call and two around it, ~2 M calls per launch.  (Arguments of a device function arrive in vector registers: made scalars again below.)
__device__ __attribute__((noinline)) WalkState walk_fast(lds_int *keys, int fmt, int use_lds, int vals_lds, unsigned mask, unsigned nslots, int *gkeys, int *gvals,
                                                         uint8_t *ub, int *us, int k, int seed, int max_steps, int backward,
                                                         int node, int l, int pend, int pend_at, int chk_node, int chk_l, int chk_pow)
{
    keys = (lds_int *)(unsigned)uni((int)(unsigned)(unsigned long long)keys);
    ub = (uint8_t *)uni64((long long)ub); us = (int *)uni64((long long)us);
    k = uni(k); seed = uni(seed); max_steps = uni(max_steps); backward = uni(backward);
    Tab t;
    t.fmt = uni(fmt); t.use_lds = uni(use_lds); t.vals_lds = uni(vals_lds); t.mask = (unsigned)uni((int)mask); t.nslots = (unsigned)uni((int)nslots);
    t.gkeys = (int *)uni64((long long)gkeys); t.gvals = (int *)uni64((long long)gvals);
    t.n_compact = -1; t.ckeys = nullptr; t.cslots = nullptr;
    WalkState w;
    w.node = uni(node); w.l = uni(l); w.pend = uni(pend); w.pend_at = uni(pend_at); w.status = WALK_RUNNING; w.fast_steps = 0;
    w.chk_node = uni(chk_node); w.chk_l = uni(chk_l); w.chk_pow = uni(chk_pow);
    {
        int nfast = 0;
#define WALK_PAIR(EARLY_, LIM_) do { \
            if (t.fmt == TAB_DIRECT) { if (backward) walk_pair_steps<TAB_DIRECT, true, EARLY_>(keys, t, ub, us, k, seed, LIM_, w); else walk_pair_steps<TAB_DIRECT, false, EARLY_>(keys, t, ub, us, k, seed, LIM_, w); } \
            else if (t.fmt == TAB_PACKED) { if (backward) walk_pair_steps<TAB_PACKED, true, EARLY_>(keys, t, ub, us, k, seed, LIM_, w); else walk_pair_steps<TAB_PACKED, false, EARLY_>(keys, t, ub, us, k, seed, LIM_, w); } \
            else if (t.use_lds) { if (backward) walk_pair_steps<TAB_SPLIT, true, EARLY_>(keys, t, ub, us, k, seed, LIM_, w); else walk_pair_steps<TAB_SPLIT, false, EARLY_>(keys, t, ub, us, k, seed, LIM_, w); } \
            else { if (backward) walk_pair_steps<TAB_SPLIT_GLOBAL, true, EARLY_>(keys, t, ub, us, k, seed, LIM_, w); else walk_pair_steps<TAB_SPLIT_GLOBAL, false, EARLY_>(keys, t, ub, us, k, seed, LIM_, w); } } while (0)
        if (w.l < 10) {
            const int lim = max_steps < 10 ? max_steps : 10;
            WALK_PAIR(true, lim);
            nfast = w.fast_steps;
        }
        if (w.status == WALK_RUNNING && w.l >= 10 && w.l < max_steps) {
            WALK_PAIR(false, max_steps);
            nfast += w.fast_steps;
        }
#undef WALK_PAIR
        w.fast_steps = nfast;
    }
    return w;
}

// Screening of seeds, one walk per LANE.  The reference tries the seeds of a (window, k, direction) one after the other
// until a walk closes (consensus.c:536-579); where none does - a repeat whose unit is longer than MAX_PERIOD, a window of
// unrelated sequence - that is up to 100 walks of up to 500 steps, one dependent step at a time (a 4.6 kb read with a
// 520-base unit: 612 000 steps = 420 ms on its wavefront).  Walks are independent, and a walk that stays on the fast path
// (unique best successor, or l < 10) needs nothing but table look-ups: after the first failed seed the remaining ones
// are walked 64 at a time, each lane doing all four look-ups of its own walk.  Result per lane: 0 = the walk fails (no
// return to the seed within max_steps, or a cycle without the seed, or period >= MAX_PERIOD), 1 = it closes, 2 = it meets
// a tie at l >= 10, which only the general look-ahead decides.  The caller skips the seeds that fail and hands the first
// other one to walk(), which produces the unit; nothing is assumed about a seed the screen could not decide.
#define MTRC_SCREEN_MIN_SEEDS 8     // fewer seeds left than this: walked one after the other as before (a screen costs about one full walk)
template <int FMT, bool BACKWARD>
DEVINL int walk_screen_steps(lds_int *keys, const Tab &t, int k, int seed, bool active, int max_steps)
{
    const int sh1 = 2 * (k - 1), p4k1 = 1 << sh1, m1 = p4k1 - 1;
    int node = seed, res = 0;
    bool run = active;
    int chk_node = -1, chk_l = -1, chk_pow = 1;
    for (int l = 0; l < max_steps; l++) {
        // done when every walk has ended, or when the first seed that does not fail is known: a lane with a result
        // 1 / 2 below which no lane is still walking (the seeds after it do not matter)
        const unsigned long long m_run = __ballot(run), m_pos = __ballot(res != 0);
        if (m_run == 0ull) break;
        if (m_pos != 0ull && (m_run & ((1ull << first_lane(m_pos)) - 1ull)) == 0ull) break;
        if (run) {
            int cnt[4]; bool more[4];
#pragma unroll
            for (int j = 0; j < 4; j++) cnt[j] = tab_get_first<FMT>(keys, t, BACKWARD ? ((j << sh1) + (node >> 2)) : (((node & m1) << 2) + j), more[j]);
            if (more[0] || more[1] || more[2] || more[3]) {
#pragma unroll
                for (int j = 0; j < 4; j++) if (more[j]) cnt[j] = tab_get_raw<FMT>(keys, t, BACKWARD ? ((j << sh1) + (node >> 2)) : (((node & m1) << 2) + j));
            }
            int bst = cnt[0], first = 0;
            if (cnt[1] > bst) { bst = cnt[1]; first = 1; }
            if (cnt[2] > bst) { bst = cnt[2]; first = 2; }
            if (cnt[3] > bst) { bst = cnt[3]; first = 3; }
            const int nf1 = (cnt[0] == bst ? 1 : 0) + (cnt[1] == bst ? 1 : 0) + (cnt[2] == bst ? 1 : 0) + (cnt[3] == bst ? 1 : 0);
            if (nf1 != 1 && l >= 10) { res = 2; run = false; }
            else {
                node = BACKWARD ? (first * p4k1 + (node >> 2)) : (4 * (node & m1) + (nf1 == 1 ? first : 0));    // as walk_pair_steps
                if (node == seed) { res = (l + 1 < MTRC_MAX_PERIOD) ? 1 : 0; run = false; }
                else if (l >= 10 && walk_cycle_check(node, l, chk_node, chk_l, chk_pow)) { res = 0; run = false; }
            }
        }
        loop_join();
    }
    return res;
}
__device__ __attribute__((noinline)) int walk_screen(lds_int *keys, Tab t, int k, int seed, int active, int max_steps, int backward)
{
    keys = (lds_int *)(unsigned)uni((int)(unsigned)(unsigned long long)keys);
    k = uni(k); max_steps = uni(max_steps); backward = uni(backward);
    t.fmt = uni(t.fmt); t.use_lds = uni(t.use_lds); t.vals_lds = uni(t.vals_lds); t.mask = (unsigned)uni((int)t.mask); t.nslots = (unsigned)uni((int)t.nslots);
    t.gkeys = (int *)uni64((long long)t.gkeys); t.gvals = (int *)uni64((long long)t.gvals);
    const bool act = active != 0;
    if (t.fmt == TAB_DIRECT) return backward ? walk_screen_steps<TAB_DIRECT, true>(keys, t, k, seed, act, max_steps) : walk_screen_steps<TAB_DIRECT, false>(keys, t, k, seed, act, max_steps);
    if (t.fmt == TAB_PACKED) return backward ? walk_screen_steps<TAB_PACKED, true>(keys, t, k, seed, act, max_steps) : walk_screen_steps<TAB_PACKED, false>(keys, t, k, seed, act, max_steps);
    return backward ? walk_screen_steps<TAB_SPLIT, true>(keys, t, k, seed, act, max_steps) : walk_screen_steps<TAB_SPLIT, false>(keys, t, k, seed, act, max_steps);
}
// index of the first seed in [s, ns) whose walk does not provably fail (ns if every one does)
DEVINL int screen_seeds(K2Ctx &c, bool backward, int qs, int qe, int k, int s, int ns)
{
    const int lane = lane_id();
    int max_steps = (qe - qs) / MTRC_MIN_NUM_FREQ_UNIT; if (max_steps > MTRC_MAX_PERIOD) max_steps = MTRC_MAX_PERIOD;
    const unsigned long long t0 = clk();
    int first = ns;
    for (int b = s; b < ns && first == ns; b += 64) {
        const int idx = b + lane;
        const bool act = idx < ns;
        const int sd = act ? (int)c.seeds[idx] : 0;
        const int r = walk_screen(c.lds_keys, c.tab, k, sd, act ? 1 : 0, max_steps, backward ? 1 : 0);
        const unsigned long long m = __ballot(act && r != 0);
        if (m != 0ull) first = b + first_lane(m);
        loop_join();
    }
    wc_time(c.wc, CYC_WALK, t0);
    return uni(first);
}

DEVINL int walk(K2Ctx &c, bool backward, int qs, int qe, int k, int seed, int dst)
{
    const int lane = lane_id();
    uint8_t *ub = slot_unit(c, dst); int *us = slot_score(c, dst);
    const int p4k1 = 1 << (2 * (k - 1));
    int period = 0;
    const unsigned long long t0 = clk();
    int max_steps = (qe - qs) / MTRC_MIN_NUM_FREQ_UNIT; if (max_steps > MTRC_MAX_PERIOD) max_steps = MTRC_MAX_PERIOD;
    long long lookups = 0;
    WalkState w; w.node = seed; w.l = 0; w.pend = 0; w.pend_at = -1; w.status = WALK_RUNNING; w.fast_steps = 0;
    w.chk_node = -1; w.chk_l = -1; w.chk_pow = 1;
    wc_add(c.wc, CNT_WALK_CALLS, 1);
    while (w.l < max_steps) {
        const unsigned long long t_fast = clk();
        w = walk_fast(c.lds_keys, c.tab.fmt, c.tab.use_lds, c.tab.vals_lds, c.tab.mask, c.tab.nslots, c.tab.gkeys, c.tab.gvals, ub, us, k, seed, max_steps, backward ? 1 : 0,
                      w.node, w.l, w.pend, w.pend_at, w.chk_node, w.chk_l, w.chk_pow);
        wc_time(c.wc, CYC_WALK_FAST, t_fast);
#ifdef MTR_PROFILE_WALK_FMT
        // development build (tests/dev/r5/walk_fmt.py): the fast steps of mtr_k_walks_k by table layout - 1: cycles, 2: steps, 3: calls
        if (c.prof_kernel == 1 && MTR_PROFILE_WALK_FMT <= 3) {
            const Tab &pt = c.tab;
            const int cls_ = pt.fmt == TAB_DIRECT ? CNT_SPARE43 : pt.fmt == TAB_PACKED ? (pt.nslots <= 1024u ? CNT_SPARE44 : CNT_SPARE45)
                             : !pt.use_lds ? CNT_SPARE55 : pt.vals_lds ? CNT_SPARE46 : CNT_SPARE47;
            if (MTR_PROFILE_WALK_FMT == 1) wc_time(c.wc, cls_, t_fast);
            else if (MTR_PROFILE_WALK_FMT == 2) wc_add(c.wc, cls_, uni(w.fast_steps));
            else wc_add(c.wc, cls_, 1);
        }
#endif
        const int l = uni(w.l);
        int node = uni(w.node), pend_score = uni(w.pend), pend_at = uni(w.pend_at);
        const int status = uni(w.status);
        lookups += 4ll * uni(w.fast_steps);
        wc_add(c.wc, CNT_WALK_STEPS, uni(w.fast_steps));
        if (status == WALK_CLOSED) { period = l + 1; if (MTRC_MAX_PERIOD <= period) period = 0; break; }
        if (status == WALK_CYCLE || l >= max_steps) break;
        // ---- one step through the general look-ahead (l >= 10 and the four successors tie) ---------------------------
        if (!backward) {                                                     // :286-293
            if (lane == 0 && l > 0) us[l - 1] = pend_score;
            pend_score = uni(tab_get(c, node));
            if (lane == 0) ub[l] = (uint8_t)(node >> (2 * (k - 1)));
            pend_at = l;
        }
        // From step 10 on the step is a function of the node alone (k levels are looked at whatever l is): the walks of
        // the other seeds of this table run into the same few nodes (dead ends, the all-A node), whose decision - a scan
        // of the whole table each - is remembered per table and direction.
        const int nsc = c.tab.use_lds ? K2_STEP_CACHE_LDS : K2_STEP_CACHE;
        int4 *sce = (int4 *)(c.sc + c.y.step_cache) + ((backward ? nsc : 0) + (int)((tab_hash(node) >> 7) & (unsigned)(nsc - 1)));
        const int from = node;
        const int4 ce = *sce;
        const int ck = uni(ce.x), cv = uni(ce.y), cg = uni(ce.z);
        if (ck == from && cg == c.tab_gen) {
            node = cv;
            if (backward) {
                if (lane == 0 && l > 0) us[l - 1] = pend_score;
                pend_score = uni(tab_get(c, node));
                if (lane == 0) ub[l] = (uint8_t)(node >> (2 * (k - 1)));
                pend_at = l;
            }
        } else {
        int m;
        const int best_digit = lookahead(c, backward, node, k, k, m, lookups);
        if (!backward) node = 4 * (node & (p4k1 - 1)) + (m - 1 >= 15 ? 0 : (best_digit >> (2 * (m - 1))));   // :335 (H6)
        else {
            node = (best_digit & 3) * p4k1 + (node >> 2);                                               // :418
            if (lane == 0 && l > 0) us[l - 1] = pend_score;
            pend_score = uni(tab_get(c, node));
            if (lane == 0) ub[l] = (uint8_t)(node >> (2 * (k - 1)));                                   // :421-426
            pend_at = l;
        }
        if (lane == 0) *sce = make_int4(from, node, c.tab_gen, 0);
        wave_sync_mem();
        }
        w.node = node; w.l = l + 1; w.pend = pend_score; w.pend_at = pend_at;
        loop_join();
        if (node == seed) { period = l + 1; if (MTRC_MAX_PERIOD <= period) period = 0; break; }
        {
            int cn = uni(w.chk_node), cl = uni(w.chk_l), cp = uni(w.chk_pow);
            const bool cyc = walk_cycle_check(node, l, cn, cl, cp);                 // general steps happen at l >= 10 only
            w.chk_node = cn; w.chk_l = cl; w.chk_pow = cp;
            if (cyc) break;
        }
    }
    const int pend_at = uni(w.pend_at), pend_score = uni(w.pend);
    if (lane == 0 && pend_at >= 0) us[pend_at] = pend_score;
    wc_add(c.wc, CNT_LOOKUPS, lookups);
    // The staged chain's walk kernels read a found unit once, when st_park_entries copies it out: that copy waits for the stores (once per range, not per walk)
    // and turns a backward unit round as it goes - here that was one memory round trip per walk and two more per backward unit.
    if (!c.staged_walks) wave_sync_mem();
    wc_time(c.wc, CYC_WALK, t0);
    // per-walk cost record (trace type 8; the cycles only in the timed build): window, k, direction, seed, steps, unit length found,
    // cycles / 1024, table look-ups of the general steps
    trace_ev(c, 8, qs, qe, k, backward ? 1 : 0, seed, uni(w.l), period, (int)((clk() - t0) >> 10), (int)(lookups > 0x7fffffffll ? 0x7fffffffll : lookups), 0, 0, 0, 0, 0);
    if (period == 0) return 0;
    wc_add(c.wc, CNT_WALK_CLOSED, 1);
    // the candidate record starts from a cleared one (clear_rr: every string_score = -1); a later revision
    // may lengthen the unit and then reports those untouched entries
    if (!c.staged_walks) for (int t = period + lane; t < K2_SLOT_SCORE; t += 64) us[t] = -1;
    if (backward && !c.staged_walks) {                                                                  // :466-476
        for (int t = lane; t < period / 2; t += 64) {
            uint8_t b0 = ub[t], b1 = ub[period - 1 - t]; ub[t] = b1; ub[period - 1 - t] = b0;
            int s0 = us[t], s1 = us[period - 1 - t]; us[t] = s1; us[period - 1 - t] = s0;
        }
        wave_sync_mem();
    }
    return period;
}

// ---------------------------------------------------------------------------------------------------------
// DP wrappers
// ---------------------------------------------------------------------------------------------------------
DEVINL void apply_dp(RR &r, int qs, const DpRes &o, int U, int G, int MM, int D)
{   // wrap_around_DP_sub's result fields (wrap_around_DP.c:338-351)
    // (the traceback's counts are wave-uniform but come out of loops with lane-dependent exits: said here, so that
    // the records of the k loop live in scalar registers instead of being spilled vector registers)
    const int stop_i = uni(o.stop_i), end_i = uni(o.end_i);
    r.rep_start = qs + stop_i + 1; r.rep_end = qs + end_i; r.repeat_len = end_i - stop_i;
    r.copies = uni(o.scanned) / U; r.mat = uni(o.mat); r.mis = uni(o.mis); r.ins = uni(o.ins); r.del = uni(o.del); r.G = G; r.MM = MM; r.D = D;
}

DEVINL bool dp_sub_unit(K2Ctx &c, int qs, int qe, RR &r, const uint8_t *unit, int G, int MM, int D)
{
    DpRes o;
    const int U = r.period;
    bool ok = dp_wrap(c.pk, qs, qe - qs + 1, unit, U, G, MM, D, c.sc + c.y.codes, c.y.cells, 0, nullptr, nullptr, nullptr, o, c.wc, c.a->dp16_max_rows);
    if (!ok) { dp_too_large(c); return false; }
    apply_dp(r, qs, o, U, G, MM, D);
    trace_ev(c, 3, qs, qe, U, trace_on(c, 3) ? unit_hash(unit, U) : 0, G, MM, D, r.rep_start, r.rep_end, r.repeat_len, r.copies, r.mat, r.mis, r.ins);
    return true;
}
DEVINL bool dp_sub(K2Ctx &c, int qs, int qe, RR &r, int slot, int G, int MM, int D) { return dp_sub_unit(c, qs, qe, r, slot_unit(c, slot), G, MM, D); }

// wrap_around_DP's result is a pure function of (window, unit): the k loop and the two walk directions of one
// range keep producing the same unit (a third of the reference's calls, ~15 % of its DP cells, repeat an earlier
// call of the same range verbatim).  The answers of the current range are remembered; a repeated unit (exact
// byte comparison, not a hash) gets its answer back without the DP.
DEVINL bool memo_lookup(K2Ctx &c, int qs, int qe, const uint8_t *ub, int U, RR &r)
{
    const int lane = lane_id();
    if (c.memo_qs != qs || c.memo_qe != qe) { c.memo_n = 0; c.memo_qs = qs; c.memo_qe = qe; return false; }
    unsigned long long m = __ballot(lane < c.memo_n && c.memo_U == U);
    while (m != 0ull) {
        const int e = first_lane(m);
        m &= m - 1ull;
        const uint8_t *mu = c.sc + c.y.memo_unit + (size_t)e * K2_MEMO_UNIT;
        bool diff = false;
        for (int t = lane; t < U; t += 64) diff = diff || (mu[t] != ub[t]);
        if (__ballot(diff) == 0ull) {
            const int *mr = (const int *)(c.sc + c.y.memo_res) + e * 16;
            const int v = lane < 13 ? mr[lane] : 0;
            RR o;
            o.rep_start = lane_val(v, 0); o.rep_end = lane_val(v, 1); o.repeat_len = lane_val(v, 2); o.period = lane_val(v, 3);
            o.copies = lane_val(v, 4); o.mat = lane_val(v, 5); o.mis = lane_val(v, 6); o.ins = lane_val(v, 7); o.del = lane_val(v, 8);
            o.kmer = lane_val(v, 9); o.G = lane_val(v, 10); o.MM = lane_val(v, 11); o.D = lane_val(v, 12);
            if (o.period != -1) { o.kmer = r.kmer; o.period = r.period; }     // a cleared record stays cleared
            r = o;
            wc_add(c.wc, CNT_MEMO_HITS, 1);
            wc_add(c.wc, CNT_MEMO_CELLS, 2ll * (long long)(qe - qs + 1) * (long long)U);
            return true;
        }
        loop_join();
    }
    return false;
}
DEVINL void memo_store(K2Ctx &c, const uint8_t *ub, int U, const RR &r)
{
    const int lane = lane_id();
    if (c.memo_n >= K2_MEMO_N || U > K2_MEMO_UNIT) return;
    const int e = c.memo_n;
    uint8_t *mu = c.sc + c.y.memo_unit + (size_t)e * K2_MEMO_UNIT;
    for (int t = lane; t < U; t += 64) mu[t] = ub[t];
    int *mr = (int *)(c.sc + c.y.memo_res) + e * 16;
    if (lane == 0) {
        mr[0] = r.rep_start; mr[1] = r.rep_end; mr[2] = r.repeat_len; mr[3] = r.period; mr[4] = r.copies; mr[5] = r.mat; mr[6] = r.mis;
        mr[7] = r.ins; mr[8] = r.del; mr[9] = r.kmer; mr[10] = r.G; mr[11] = r.MM; mr[12] = r.D;
    }
    if (lane == e) c.memo_U = U;
    c.memo_n = e + 1;
    wave_sync_mem();
}

// wrap_around_DP (wrap_around_DP.c:357-429): (1,1,3) then (1,3,1); strictly better float ratio wins.  `unit` may lie
// anywhere in global memory (the staged mode aligns candidates parked in HBM); no memo here.
DEVINL void dp_two_params_unit(K2Ctx &c, int qs, int qe, RR &r, const uint8_t *unit)
{
    RR best; rr_clear(best);
    float best_ratio = -1.0f;
    const int U = r.period;
    if (dp_wrap2_fits(qe - qs + 1, U, c.a->dp16_max_rows)) {
        // both parameter sets in one forward pass
        DpRes o[2];
        bool ok = dp_wrap2(c.pk, qs, qe - qs + 1, unit, U, 1, 1, 3, 1, 3, 1, c.sc + c.y.codes, c.y.cells, o, c.wc, c.a->dp16_max_rows);
        if (!ok) { dp_too_large(c); r = best; return; }
        for (int p = 0; p < 2; p++) {
            RR t = r;
            apply_dp(t, qs, o[p], U, 1, p == 0 ? 1 : 3, p == 0 ? 3 : 1);
            trace_ev(c, 3, qs, qe, U, trace_on(c, 3) ? unit_hash(unit, U) : 0, 1, p == 0 ? 1 : 3, p == 0 ? 3 : 1, t.rep_start, t.rep_end, t.repeat_len, t.copies, t.mat, t.mis, t.ins);
            float q = rr_ratio(t);
            if (best_ratio < q) { best = t; best_ratio = q; }
        }
        r = best;
        return;
    }
    RR t = r;
    if (dp_sub_unit(c, qs, qe, t, unit, 1, 1, 3)) { float q = rr_ratio(t); if (best_ratio < q) { best = t; best_ratio = q; } }
    t = r;
    if (dp_sub_unit(c, qs, qe, t, unit, 1, 3, 1)) { float q = rr_ratio(t); if (best_ratio < q) { best = t; best_ratio = q; } }
    r = best;
}
DEVINL void dp_two_params(K2Ctx &c, int qs, int qe, RR &r, int slot)
{
    const int U = r.period;
    if (memo_lookup(c, qs, qe, slot_unit(c, slot), U, r)) return;
    dp_two_params_unit(c, qs, qe, r, slot_unit(c, slot));
    memo_store(c, slot_unit(c, slot), U, r);
}

DEVINL void pool_store(K2Ctx &c, int e, const RR &r)
{
    int *pr = (int *)(c.sc + c.y.pool_res) + e * 16;
    if (lane_id() == 0) {
        pr[0] = r.rep_start; pr[1] = r.rep_end; pr[2] = r.repeat_len; pr[3] = r.period; pr[4] = r.copies; pr[5] = r.mat; pr[6] = r.mis;
        pr[7] = r.ins; pr[8] = r.del; pr[9] = r.kmer; pr[10] = r.G; pr[11] = r.MM; pr[12] = r.D;
    }
}
DEVINL void pool_load(K2Ctx &c, int e, RR &o)
{
    const int lane = lane_id();
    const int *pr = (const int *)(c.sc + c.y.pool_res) + e * 16;
    const int v = lane < 13 ? pr[lane] : 0;
    o.rep_start = lane_val(v, 0); o.rep_end = lane_val(v, 1); o.repeat_len = lane_val(v, 2); o.period = lane_val(v, 3);
    o.copies = lane_val(v, 4); o.mat = lane_val(v, 5); o.mis = lane_val(v, 6); o.ins = lane_val(v, 7); o.del = lane_val(v, 8);
    o.kmer = lane_val(v, 9); o.G = lane_val(v, 10); o.MM = lane_val(v, 11); o.D = lane_val(v, 12);
}

// wrap_around_DP of up to four candidates of one range whose units have at most 16 bases, in ONE forward pass
// (dp_forward2p_q4): `ents` = their pool entries, 5 bits each.  Each result goes through the same selection between the
// two parameter sets as dp_two_params, into the memo and into the pool.
DEVINL bool dp_batch_fits(const K2Ctx &c, int rows)
{
    return rows <= DP2P_MAX_ROWS && rows <= c.a->dp16_max_rows && (size_t)4 * 16 * (size_t)rows <= c.y.cells && dp_size_ok(16, rows);   // (beyond WrapDPsize: one by one, dp_wrap2 says which)
}
// The pass itself for up to four units (q.n, q.U, q.unit; kk = their k): forward pass, the two tracebacks of each and the
// selection between the two parameter sets; store(g, record, ok) receives each result (ok = false: a traceback found the
// matrix corrupt, the record is cleared).  Callers: the per-read kernel's pool (below), the staged chain's alignment kernel.
// (The slot filling below - matrices one behind the other, a DP that is not there with one column and no cells - is written out once more in
//  mtr_k_dp_test_waves, dp_test.hip.inc, which needs each parameter set's result: change both together.)
template <typename F>
DEVINL void dp_two_params_q4(K2Ctx &c, int qs, int qe, Dp4 &q, const int (&kk)[4], F &&store)
{
    const int rows = qe - qs + 1, n = q.n;
    size_t off = 0;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const bool on = g < n;
        if (!on) { q.U[g] = 1; q.unit[g] = q.unit[0]; }
        q.off[g] = on ? off : 0;
        if (on) off += (size_t)rows * (size_t)q.U[g];
    }
    uint8_t *codes = c.sc + c.y.codes;
    int best[4][2][3];
    const unsigned long long t_f = clk();
    dp_forward2p_q4(c.pk, qs, rows, q, 1, 1, 3, 1, 3, 1, codes, best);
    wave_sync_mem();
    wc_time(c.wc, CYC_DP_FWD, t_f);
    wc_time_aux(c.wc, CNT_SPARE47, t_f);
    const unsigned long long t_b = clk();
#pragma unroll
    for (int g = 0; g < 4; g++) {
        if (g < n) {
            const int U = q.U[g];
            RR r; rr_clear(r); r.period = U; r.kmer = kk[g];
            RR bestr; rr_clear(bestr);
            float best_ratio = -1.0f;
            long long tb = 0;
            bool ok = true;
            for (int p = 0; p < 2; p++) {
                DpRes o; o.stop_i = 0; o.end_i = 0; o.mat = o.mis = o.ins = o.del = o.scanned = 0; o.end_j = 0;
                const int bv = uni(best[g][p][0]), bi = uni(best[g][p][1]), bj = uni(best[g][p][2]);
                if (bv > 0) {
                    dp_traceback<0, 1>(c.pk, qs, U, codes + q.off[g], p, U, bi, bj, nullptr, nullptr, nullptr, o, c.wc);
                    if (o.stop_i < 0) { o.stop_i = 0; o.end_i = 0; o.mat = o.mis = o.ins = o.del = o.scanned = 0; ok = false; }
                }
                tb += (long long)(o.mat + o.mis + o.ins + o.del);
                RR t = r;
                apply_dp(t, qs, o, U, 1, p == 0 ? 1 : 3, p == 0 ? 3 : 1);
                trace_ev(c, 3, qs, qe, U, trace_on(c, 3) ? unit_hash(q.unit[g], U) : 0, 1, p == 0 ? 1 : 3, p == 0 ? 3 : 1, t.rep_start, t.rep_end, t.repeat_len, t.copies, t.mat, t.mis, t.ins);
                const float qq = rr_ratio(t);
                if (best_ratio < qq) { bestr = t; best_ratio = qq; }
                loop_join();
            }
            if (!ok) { dp_too_large(c); rr_clear(bestr); }
            store(g, bestr, ok);
            if (lane_id() == 0) {
                c.wc[CNT_DP_CALLS] += 2ull; c.wc[CNT_DP_CELLS] += 2ull * (unsigned long long)rows * (unsigned long long)U;
                c.wc[CNT_DP_ROWS] += 2ull * (unsigned long long)rows; c.wc[CNT_TB_STEPS] += (unsigned long long)tb;
            }
        }
    }
    wc_time(c.wc, CYC_DP_TB, t_b);
}
DEVINL void dp_two_params_batch(K2Ctx &c, int qs, int qe, int n, unsigned ents)
{
    const int *pmeta = (const int *)(c.sc + c.y.pool_meta);
    Dp4 q; q.n = n;
    int ent[4], kk[4];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        ent[g] = (int)((ents >> (5 * g)) & 31u);
        const int e = g < n ? ent[g] : ent[0];
        q.U[g] = g < n ? uni(pmeta[4 * e]) : 1;
        kk[g] = uni(pmeta[4 * e + 1]);
        q.unit[g] = slot_unit(c, K2_NSLOT_FIXED + e);
        q.off[g] = 0;
    }
    dp_two_params_q4(c, qs, qe, q, kk, [&](int g, const RR &bestr, bool ok) {
        if (ok) memo_store(c, q.unit[g], q.U[g], bestr);
        pool_store(c, ent[g], bestr);
    });
}
// the bases of a unit of at most 16 bases as one word (bit j = bit 0 of base j, bit 16 + j = bit 1 of base j)
DEVINL unsigned unit_key16(const uint8_t *ub, int U)
{
    const int lane = lane_id();
    const int b = lane < U ? (int)ub[lane] : 0;
    const unsigned lo = (unsigned)__ballot((b & 1) != 0), hi = (unsigned)__ballot((b & 2) != 0);
    return (lo & 0xffffu) | (hi << 16);
}

// ---------------------------------------------------------------------------------------------------------
// search_De_Bruijn_graph (consensus.c:507-582), first half: table, seeds and walks of one k.  A unit a walk finds is left
// in pool slot K2_NSLOT_FIXED + n_ent and listed in the range's candidate list (its DP comes later, k2_range); e_of[dir]
// = its entry, -1 = none.  Returns the found flag of the LAST attempt (SURVEY H4).
// ---------------------------------------------------------------------------------------------------------
DEVINL int search_walks(K2Ctx &c, int qs, int qe, int k, int &max_freq_out, int &n_ent, int (&e_of)[2])
{
    const int lane = lane_id();
    int max_freq = tab_build(c, k, qs, qe);
    max_freq_out = max_freq;
    int found = 0;
    e_of[0] = -1; e_of[1] = -1;
    int *pmeta = (int *)(c.sc + c.y.pool_meta);
    if (MTRC_MIN_NUM_FREQ_UNIT < max_freq) {
        int ns = tab_seeds(c, k, qs, qe, max_freq);
        // The reference searches forward, then backward, and keeps the found flag of the LAST attempt (H4): a k whose
        // backward search closes no walk is dropped whatever the forward search found.  The two searches do not depend on
        // each other, so the backward one runs first and the forward one only if it matters.
        int found_bwd = 0;
        for (int turn = 0; turn < 2; turn++) {
            const int dir = 1 - turn;
            if (turn == 1 && !found_bwd) break;
            for (int s = 0; s < ns; s++) {
                int seed = uni(c.seeds[s]);
                int period = walk(c, dir == 1, qs, qe, k, seed, K2_NSLOT_FIXED + n_ent);
                found = period > 0 ? 1 : 0;
                if (!found && s + MTRC_SCREEN_MIN_SEEDS < ns) {
                    // the seeds after a failed one are screened 64 at a time; those that provably fail are not walked
                    // (found stays 0, the flag of the last attempt); the loop goes on with the first other one
                    s = screen_seeds(c, dir == 1, qs, qe, k, s + 1, ns) - 1;
                }
                if (found) {
                    if (period < MTRC_MIN_PERIOD) {
                        // a one-base unit can never be chosen (MIN_PERIOD <= period, consensus.c:562-566), whatever its
                        // alignment says: the reference's two DPs for it (5 % of its DP rows on 2 kb reads) are not run
                        wc_add(c.wc, CNT_MEMO_HITS, 1);
                        wc_add(c.wc, CNT_MEMO_CELLS, 2ll * (long long)(qe - qs + 1) * (long long)period);
                        break;
                    }
                    if (lane == 0) { pmeta[4 * n_ent] = period; pmeta[4 * n_ent + 1] = k; pmeta[4 * n_ent + 2] = dir; }
                    e_of[dir] = n_ent;
                    n_ent++;
                    break;
                }
                loop_join();
            }
            if (dir == 1) found_bwd = found;
            loop_join();
        }
        found = found_bwd;
    }
    return found;
}


// ---------------------------------------------------------------------------------------------------------
// polish_repeat (consensus.c:610-704): operates on RR r / slot 1 in place
// ---------------------------------------------------------------------------------------------------------
// The unit and its node frequencies are staged in LDS, one byte per position (polish_plan.h: pp_stage_byte; bits 0-1 = base, bits 2-3 =
// min(string_score, 3) - the walk only asks "== 1" and "< 2").  Read from global scratch each of a position's ~2-10 look-ups was a
// dependent 1-2 us round trip.  The polished unit is written into the bytes behind them (out[jr], jr = MTRC_MAX_PERIOD - 1 downwards).
// The walk itself is polish_plan.h's: every lane answers the flag predicate for its own positions, ballots make the flagged set, and the
// walk visits the flagged positions only (pp_walk_plan) - the stretches between them are copies, 64 bases a store.
// -DMTR_POLISH_WALK_ALL (a build of its own, for A/B runs; never a runtime switch): the reference's walk over every position (pp_walk_all).
#define POL_OUT_OFF 512                      // the output's bytes within c.stage (1024 bytes, free here: no look-ahead runs during polish)
static_assert(MTRC_MAX_PERIOD <= POL_OUT_OFF, "a staged unit and its polished form share the look-ahead's staging bytes");
DEVINL int pol_base(const lds_u8 *st, int j) { return uni((int)st[j]) & 3; }               // everything in the walk is wave-uniform: say so (uni)
DEVINL int pol_score(const lds_u8 *st, int j) { return (uni((int)st[j]) >> 2) & 3; }
// this wavefront's LDS writes before its later LDS reads from other lanes (a wavefront's LDS operations run in order: the compiler must keep them so)
DEVINL void wave_sync_lds()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}
struct PolMask {                             // polish_plan.h's flagged set on a wavefront: lane q holds word q
    long long v;
    DEVINL unsigned long long word(int q) const { return (unsigned long long)lane_val64(v, q); }
};
struct PolOps {                              // polish_plan.h's OPS on a wavefront
    const K2Ctx *c; const lds_u8 *st; lds_u8 *out; int k, period;
    DEVINL int base(int j) const { return pol_base(st, j); }
    DEVINL int score(int j) const { return pol_score(st, j); }
    DEVINL int get(int node) const { return uni(tab_get(*c, node)); }
    // four look-ups side by side, lane l asks for the l-th node: one trip to the table instead of four in a row
    DEVINL void get4(int a0, int a1, int a2, int a3, int &f0, int &f1, int &f2, int &f3) const
    {
#ifdef MTR_POLISH_WALK_ALL
        f0 = get(a0); f1 = get(a1); f2 = get(a2); f3 = get(a3);
#else
        const int lane = lane_id();
        const int key = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
        int v = 0;
        if (lane < 4) v = tab_get(*c, key);
        f0 = lane_val(v, 0); f1 = lane_val(v, 1); f2 = lane_val(v, 2); f3 = lane_val(v, 3);
#endif
    }
    // the cyclic k-mer at j with one ballot: lane l answers bit l of the node, bit l & 1 of the base k - 1 - (l >> 1) places behind j
    DEVINL int cyc(int j) const
    {
        const int lane = lane_id();
        const bool on = lane < 2 * k;
        int pos = j + (k - 1 - (lane >> 1)); if (pos >= period) pos -= period;                 // (period > k: one wrap at most)
        const int b = on ? (int)st[pos] : 0;
        return (int)(unsigned)__ballot(on && ((b >> (lane & 1)) & 1) != 0);
    }
    DEVINL void emit(int jr, int b) const { if (lane_id() == 0) out[jr] = (unsigned char)b; }
    DEVINL void copy(int jr, int j, int n) const
    {   // (not unrolled: at most eight rounds, and an unrolled copy took thirty-odd registers for its bytes in flight)
#pragma unroll 1
        for (int t = j - n + 1 + lane_id(); t <= j; t += 64) out[jr - j + t] = (unsigned char)(st[t] & 3);
    }
    DEVINL void undefined() const { wc_add(c->wc, CNT_UNDEFINED, 1); }
    DEVINL void join() const { loop_join(); }
};
// polish_repeat on a staged unit (st[0 .. r.period), written by the caller and synchronised): true = the unit changed, its new form is
// out[jr + 1 .. MTRC_MAX_PERIOD - 1]; false = it stays as it is (no flagged position, a walk that altered nothing, or an output beyond
// MTRC_MAX_PERIOD, :645).  The k-mer table of the repeat (:617-619) is built only if a position is flagged.
DEVINL bool polish_staged(K2Ctx &c, const RR &r, const lds_u8 *st, lds_u8 *out, int &jr, unsigned long long t_stage)
{
    const int lane = lane_id();
    const int k = r.kmer, period = r.period;
    // The walk only ever leaves the unit's own base and a step of one at a position whose node frequency is 1 AND that is suspicious
    // (:629-631); everything else copies the unit.  If no position is flagged the unit comes out as it went in and neither the table nor
    // the walk is needed (most revisions: SURVEY appendix B, 467 of 4 538 units change).
    PolMask m; m.v = 0ll;
    unsigned long long any = 0ull;
#pragma unroll 1
    for (int q = 0; q * 64 < period; q++) {
        const int t = q * 64 + lane;
        const unsigned long long w = __ballot(t < period && pp_flagged([&](int p) { return ((int)st[p] >> 2) & 3; }, k, t));
        if (lane == q) m.v = (long long)w;
        any |= w;
    }
    const bool none = any == 0ull;
    wc_time_pol(c.wc, CNT_SPARE45, t_stage);
    if (none) return false;
    const unsigned long long t_tab = clk();
    (void)tab_build(c, k, r.rep_start, r.rep_end);             // init_inputString + generate_freqNode_return_maxNode (:617-619)
    wc_time_pol(c.wc, CNT_SPARE46, t_tab);
    const unsigned long long t_walk = clk();
    PolOps ops{&c, st, out, k, period};
    bool altered = false;
#ifdef MTR_POLISH_WALK_ALL
    const bool ok = pp_walk_all(ops, k, period, jr, altered);
#else
    const bool ok = pp_walk_plan(ops, m, k, period, jr, altered);
#endif
    wave_sync_lds();
    wc_time_pol(c.wc, CNT_SPARE47, t_walk);
    return ok && altered;
}

// RR r / unit slot `slot` in place (the per-read kernel, mtr_k_revise)
DEVINL void polish(K2Ctx &c, RR &r, int slot = 1)
{
    const int lane = lane_id();
    const int k = r.kmer, period = r.period;
    if (period <= k) return;
    uint8_t *ub = slot_unit(c, slot); const int *score = slot_score(c, slot);
    lds_u8 *st = (lds_u8 *)c.stage, *out = st + POL_OUT_OFF;
    const unsigned long long t_stage = clk();
#pragma unroll 1
    for (int t = lane; t < period; t += 64) st[t] = pp_stage_byte((int)ub[t], score[t]);
    wave_sync_lds();
    int jr = 0;
    if (!polish_staged(c, r, st, out, jr, t_stage)) return;
    const int np = (MTRC_MAX_PERIOD - 1) - jr;
#pragma unroll 1
    for (int t = lane; t < np; t += 64) ub[t] = out[t + jr + 1];
    wave_sync_mem();
    r.period = np;
}

DEVINL int min_missing(int period, double err, int coverage)
{   // consensus.c:777-820; table = consensus.c:714-775 (packed, see min_missing_table.h)
    int a = period > 200 ? 0 : period > 150 ? 1 : period > 100 ? 2 : period > 75 ? 3 : period > 50 ? 4 :
            period > 30 ? 5 : period > 20 ? 6 : period > 10 ? 7 : period > 5 ? 8 : 9;
    int b = err > 0.25 ? 0 : err > 0.225 ? 1 : err > 0.2 ? 2 : err > 0.175 ? 3 : err > 0.15 ? 4 :
            err > 0.125 ? 5 : err > 0.1 ? 6 : err > 0.075 ? 7 : err > 0.05 ? 8 : 9;
    int cc = coverage <= 1 ? 0 : coverage >= 20 ? 19 : coverage - 1;
    return (int)d_min_missing[(a * 10 + b) * 20 + cc] - '0';
}

// the threshold of the missing-base votes (consensus.c:905-916): the only way a record's error counts enter a round
DEVINL int revise_threshold(const RR &t)
{
    if (t.period <= 0) return 0x7fffffff;
    const int coverage = t.repeat_len / t.period;
    if (!(5 <= coverage && coverage <= 20)) return 0x7fffffff;
    return min_missing(t.period, (double)(t.mis + t.ins + t.del) / (double)t.repeat_len, coverage);
}
// the second half of revise_representative_unit_sub (consensus.c:964-1012): the revised unit from the votes of the traceback
// (lv: in LDS, else cons / miss in global scratch), written over unit slot `slot`; t.period becomes its length.
DEVINL void revise_tally(K2Ctx &c, RR &t, int U, lds_int *lv, const int *cons, const int *miss, int slot, bool &unchanged)
{
    const int lane = lane_id();
    uint8_t *ub = slot_unit(c, slot);
    const unsigned long long t0 = clk();
    const int thr = revise_threshold(t);
    // per column: majority base (first maximum wins, gap drops the column) + most-missing base (:964-1010)
    int *rev = (int *)(c.sc + c.y.pol_rev);     // temporary output (<= 2U entries)
    int n = 0;
    for (int base = 1; base <= U; base += 64) {
        int j = base + lane;
        int e0 = -1, e1 = -1;
        if (j <= U) {
            int mv = -1, mb = -1;
            for (int q = 0; q < 5; q++) { int v = lv ? lv[j * 5 + q] : cons[j * 5 + q]; if (mv < v) { mv = v; mb = q; } }
            if (mb < 4) e0 = mb;
            mv = -1; int mm = -1;
            for (int q = 0; q < 4; q++) { int v = lv ? lv[(U + 1) * 5 + j * 4 + q] : miss[j * 4 + q]; if (mv < v) { mv = v; mm = q; } }
            if (thr != 0x7fffffff && thr <= mv && 0 <= mm && mm <= 3) e1 = mm;
        }
        int cntl = (e0 >= 0 ? 1 : 0) + (e1 >= 0 ? 1 : 0);
        int pre = cntl;
        for (int d = 1; d < 64; d <<= 1) { int o2 = __shfl_up(pre, d, 64); if (lane >= d) pre += o2; }
        int pos = n + pre - cntl;
        if (e0 >= 0) { rev[pos] = e0; pos++; }
        if (e1 >= 0) rev[pos] = e1;
        n += lane_val(pre, 63);
    }
    wave_sync_mem();
    bool diff = false;
    for (int tt = lane; tt < n && tt < K2_SLOT_UNIT; tt += 64) { diff = diff || (ub[tt] != (uint8_t)rev[tt]); ub[tt] = (uint8_t)rev[tt]; }
    unchanged = (n == U) && (__ballot(diff) == 0ull);
    wc_add(c.wc, CNT_SPARE44, 1);
    if (unchanged) wc_add(c.wc, CNT_SPARE43, 1);
    wave_sync_mem();
    t.period = n;
    wc_time(c.wc, CYC_REVISE_VOTE, t0);
}
// revise_representative_unit_sub (consensus.c:851-1046): RR t / unit slot `slot` in place
// `dp` returns the DP of the INPUT unit; `unchanged` tells whether the votes left the unit as it was: the
// re-alignment that follows (same window, same unit, same scores) would then repeat this very DP, so the caller takes
// its result from `dp`.
DEVINL bool revise_sub(K2Ctx &c, RR &t, int G, int MM, int D, DpRes &dp, bool &unchanged, int slot = 3)
{
    const int U = t.period, rs = t.rep_start, re = t.rep_end;
    t.G = G; t.MM = MM; t.D = D;
    int *cons = (int *)(c.sc + c.y.cons), *miss = (int *)(c.sc + c.y.miss);
    uint8_t *ub = slot_unit(c, slot);
    DpRes o;
    // the votes of the traceback go to LDS when they fit (the k-mer table's arena is idle during the revision)
    lds_int *lv = ((U + 1) * 9 <= K2_TAB_CAP) ? c.lds_keys : (lds_int *)nullptr;
    bool okdp = dp_wrap(c.pk, rs, re - rs + 1, ub, U, G, MM, D, c.sc + c.y.codes, c.y.cells, 1, cons, miss, lv, o, c.wc, c.a->dp16_max_rows);
    if (!okdp) { dp_too_large(c); return false; }
    revise_tally(c, t, U, lv, cons, miss, slot, unchanged);
    dp = o;
    trace_ev(c, 5, rs, re, U, G, MM, D, t.period, trace_on(c, 5) && t.period > 0 && t.period < K2_SLOT_UNIT ? unit_hash(ub, t.period) : 0, 0, 0, 0, 0, 0, 0);
    return true;
}

// One round of revise_representative_unit (vote DP, revised unit, re-alignment) is a pure function of its parameters, the
// unit it starts from, rep_start / rep_end and the threshold above (a coarse table look-up of the error ratio): the k
// of a range often polish to the same unit over the same repeat, and their rounds repeat each other (23 % of the vote DPs
// of 2 kb reads).  A round's answer - whether it produced a candidate, the candidate's fields, the revised unit - is
// remembered per range; whether the candidate is ACCEPTED depends on the record's own ratio and stays with the caller.
DEVINL bool round_lookup(K2Ctx &c, int p, RR &t, int &valid)
{
    const int lane = lane_id();
    const int U = t.period;
    if (U <= 0 || U > K2_MEMO_UNIT) return false;
    const uint8_t *ub = slot_unit(c, 3);
    const int thr = revise_threshold(t);
    for (int e = 0; e < c.rmemo_n; e++) {
        const int *kk = (const int *)(c.sc + c.y.rmemo_key) + e * 16;
        const int mine = lane == 0 ? p : lane == 1 ? t.rep_start : lane == 2 ? t.rep_end : lane == 3 ? U : thr;
        const bool kdiff = lane < 5 && kk[lane] != mine;
        if (__ballot(kdiff) != 0ull) continue;
        const uint8_t *mu = c.sc + c.y.rmemo_kunit + (size_t)e * K2_MEMO_UNIT;
        bool diff = false;
        for (int tt = lane; tt < U; tt += 64) diff = diff || (mu[tt] != ub[tt]);
        if (__ballot(diff) != 0ull) continue;
        const int *vv = (const int *)(c.sc + c.y.rmemo_val) + e * 16;
        const int v = lane < 16 ? vv[lane] : 0;
        valid = lane_val(v, 13);
        if (valid) {
            t.rep_start = lane_val(v, 0); t.rep_end = lane_val(v, 1); t.repeat_len = lane_val(v, 2); t.period = lane_val(v, 3);
            t.copies = lane_val(v, 4); t.mat = lane_val(v, 5); t.mis = lane_val(v, 6); t.ins = lane_val(v, 7); t.del = lane_val(v, 8);
            t.G = lane_val(v, 10); t.MM = lane_val(v, 11); t.D = lane_val(v, 12);
            const uint32_t *su = (const uint32_t *)(c.sc + c.y.rmemo_vunit + (size_t)e * K2_SLOT_UNIT); uint32_t *du = (uint32_t *)slot_unit(c, 3);
            for (int tt = lane; tt < K2_SLOT_UNIT / 4; tt += 64) du[tt] = su[tt];
            wave_sync_mem();
        }
        wc_add(c.wc, CNT_MEMO_HITS, 1);
        wc_add(c.wc, CNT_MEMO_CELLS, (long long)(((unsigned long long)(unsigned)lane_val(v, 15) << 32) | (unsigned)lane_val(v, 14)));   // the cells of the round not run
        return true;
    }
    return false;
}
// revise_representative_unit (consensus.c:1048-1087): RR r / slot 1
DEVINL void revise(K2Ctx &c, RR &r)
{
    const int lane = lane_id();
    const int in_period = r.period;
    const unsigned long long t0 = clk();
    polish(c, r);
    wc_time(c.wc, CYC_POLISH, t0);
    trace_ev(c, 4, r.rep_start, r.rep_end, r.kmer, in_period, r.period, trace_on(c, 4) ? unit_hash(slot_unit(c, 1), r.period) : 0, 0, 0, 0, 0, 0, 0, 0, 0);
    const float base_ratio = rr_ratio(r);                     // not refreshed between the rounds (H7)
    for (int p = 0; p < 2; p++) {
        const int G = p == 0 ? 5 : 1, MM = 1, D = p == 0 ? 1 : 3;
        RR t = r; slot_copy(c, 3, 1);
        int valid = 0;
        if (!round_lookup(c, p, t, valid)) {
            const int me = (c.rmemo_n < K2_RMEMO_N && t.period > 0 && t.period <= K2_MEMO_UNIT) ? c.rmemo_n : -1;   // the entry this round fills
            if (me >= 0) {
                int *kk = (int *)(c.sc + c.y.rmemo_key) + me * 16;
                const int thr = revise_threshold(t);
                if (lane == 0) { kk[0] = p; kk[1] = t.rep_start; kk[2] = t.rep_end; kk[3] = t.period; kk[4] = thr; }
                const uint8_t *ub = slot_unit(c, 3); uint8_t *mu = c.sc + c.y.rmemo_kunit + (size_t)me * K2_MEMO_UNIT;
                for (int tt = lane; tt < t.period; tt += 64) mu[tt] = ub[tt];
            }
            wave_sync_mem();
            const unsigned long long cells_before = c.wc[CNT_REV_CELLS] + c.wc[CNT_MEMO_CELLS];
            DpRes dp_in; bool unchanged;
            if (revise_sub(c, t, G, MM, D, dp_in, unchanged) && t.period < MTRC_MAX_PERIOD) {
                if (t.period <= 0) wc_add(c.wc, CNT_UNDEFINED, 1);            // the reference divides by zero here
                else if (unchanged) {
                    const int qs0 = t.rep_start;
                    wc_add(c.wc, CNT_MEMO_HITS, 1);
                    wc_add(c.wc, CNT_MEMO_CELLS, (long long)(t.rep_end - qs0 + 1) * (long long)t.period);
                    apply_dp(t, qs0, dp_in, t.period, G, MM, D);              // wrap_around_DP_sub of the same unit: done above
                    valid = 1;
                } else if (dp_sub(c, t.rep_start, t.rep_end, t, 3, G, MM, D)) valid = 1;
            }
            if (me >= 0) {
                wave_sync_mem();
                int *vv = (int *)(c.sc + c.y.rmemo_val) + me * 16;
                if (lane == 0) {
                    vv[0] = t.rep_start; vv[1] = t.rep_end; vv[2] = t.repeat_len; vv[3] = t.period; vv[4] = t.copies; vv[5] = t.mat; vv[6] = t.mis;
                    vv[7] = t.ins; vv[8] = t.del; vv[9] = 0; vv[10] = t.G; vv[11] = t.MM; vv[12] = t.D; vv[13] = valid;
                    const unsigned long long cells = c.wc[CNT_REV_CELLS] + c.wc[CNT_MEMO_CELLS] - cells_before;
                    vv[14] = (int)(unsigned)(cells & 0xffffffffull); vv[15] = (int)(unsigned)(cells >> 32);
                }
                if (valid) {
                    const uint32_t *su = (const uint32_t *)slot_unit(c, 3); uint32_t *du = (uint32_t *)(c.sc + c.y.rmemo_vunit + (size_t)me * K2_SLOT_UNIT);
                    for (int tt = lane; tt < K2_SLOT_UNIT / 4; tt += 64) du[tt] = su[tt];
                }
                wave_sync_mem();
                c.rmemo_n = me + 1;
            }
        }
        if (valid && base_ratio < rr_ratio(t)) { r = t; slot_copy(c, 1, 3); wc_add(c.wc, p == 0 ? CNT_SPARE45 : CNT_SPARE46, 1); }
        loop_join();
    }
}

DEVINL void emit_record_from(const RR &r, const uint8_t *ub, const int *us, DevRecord *o)
{
    const int lane = lane_id();
    if (lane == 0) {
        o->f[0] = r.rep_start; o->f[1] = r.rep_end; o->f[2] = r.repeat_len; o->f[3] = r.period; o->f[4] = r.copies;
        o->f[5] = r.mat; o->f[6] = r.mis; o->f[7] = r.ins; o->f[8] = r.del; o->f[9] = r.kmer; o->f[10] = r.G; o->f[11] = r.MM;
        o->f[12] = r.D; o->f[13] = 0;
    }
    const int U = r.period < MTRC_MAX_PERIOD ? r.period : MTRC_MAX_PERIOD - 1;
    for (int t = lane; t < MTRC_MAX_PERIOD + 4; t += 64) o->unit[t] = t < U ? "ACGT"[ub[t] & 3] : (char)0;
    for (int t = lane; t < MTRC_MAX_PERIOD; t += 64) o->unit_score[t] = t < U ? us[t] : -1;
}
DEVINL void emit_record_to(K2Ctx &c, const RR &r, DevRecord *o) { emit_record_from(r, slot_unit(c, 0), slot_score(c, 0), o); }
DEVINL void emit_record(K2Ctx &c, const RR &r, int nrec)
{
    if (nrec >= c.a->max_rec_per_read) return;        // no slot left: only counted; the host reruns the read with more room
    const int64_t base = c.a->rec_base ? uni64(c.a->rec_base[c.rd]) : (int64_t)c.rd * (int64_t)c.a->max_rec_per_read;
    emit_record_to(c, r, c.a->records + base + nrec);
}

// One candidate range: the best unit over k (find_tandem_repeat, handle_one_read.c:102-154); true if it qualifies as
// a record (:239-240).  Result in `best`, unit and scores in slot 0.  Depends on nothing but the read and (qs, qe, w).
// The reference interleaves, k after k: table + walks, the candidates' DPs, selection, revision.  A walk depends on
// nothing a DP computes, so the three are run as PHASES over all k of the range: (1) tables, seeds and walks, the units
// found going to pool slots; (2) the DPs of the candidates (memo first); (3) per k, in the reference's order, the
// selection among the two directions (search_De_Bruijn_graph :556-571), find_tandem_repeat_sub's checks and revision
// (handle_one_read.c:84-99), and the comparison over k (:136-146).  Same results, and phase 2 sees every alignment of
// the range at once.
// what phase 1 of a range leaves behind: the k that were searched, whose last walk closed, and the pool entries of the
// candidates (5 bits per k and direction, 31 = none)
struct RangeP1 { int min_k, max_k, n_ent; unsigned run_mask, found_mask; unsigned long long ent[2]; };

// ---- phase 1: tables, seeds and walks of every k of the range; the units found go to pool slots -----------------------
// (k range of a window: k2_k_range, walk_screen.h)
// [k_from, k_to] restricts the search to some of the window's k (the staged mode spreads them over work items); bound_in =
// the smallest maximum frequency seen at smaller k (an upper bound for every larger k, below), bound_out = the same after.
DEVINL void k2_range_walks(K2Ctx &c, int qs, int qe, int w, RangeP1 &st, int k_from = 0, int k_to = 0x7fffffff,
                           int bound_in = 0x3fffffff, int *bound_out = nullptr)
{
    int min_k, max_k;
    k2_k_range(w, min_k, max_k);
    // A k whose most frequent node occurs <= MIN_NUM_FREQ_UNIT times yields nothing (consensus.c:532).  The
    // count of a (k+1)-mer never exceeds the count of its k-mer prefix at the same positions, so the smallest
    // maximum seen so far bounds every larger k; only the window's trailing raw-base nodes (SURVEY H5: positions
    // >= min(qe, L-k+1) are counted as base codes) can add to it, one each.  When bound + raw nodes <= 5 the table
    // need not be built: the result is the cleared record either way.
    int freq_bound = bound_in;
    int n_ent = 0;
    unsigned run_mask = 0u, found_mask = 0u;                          // bit k - min_k: the k was searched / its last walk closed
    unsigned long long ent[2] = { ~0ull, ~0ull };                     // 5 bits per k: candidate entry of the direction, 31 = none
    const int k0 = k_from > min_k ? k_from : min_k, k1 = k_to < max_k ? k_to : max_k;
    for (int k = k0; k <= k1; k++) {
        const int lim = qe < c.L - k + 1 ? qe : c.L - k + 1;
        const int n_raw = qe - lim + 1;
        if (freq_bound + n_raw <= MTRC_MIN_NUM_FREQ_UNIT) {
            wc_add(c.wc, CNT_TABLES_SKIPPED, 1);
            trace_ev(c, 2, qs, qe, k, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1);      // the search's answer all the same: no walk, the cleared record
            continue;
        }
        const int ki = k - min_k;
        int max_freq, e_of[2];
        const int found = search_walks(c, qs, qe, k, max_freq, n_ent, e_of);
        if (max_freq < freq_bound) freq_bound = max_freq;
        run_mask |= 1u << ki;
        if (found) found_mask |= 1u << ki;
        for (int d = 0; d < 2; d++) if (e_of[d] >= 0) ent[d] = (ent[d] & ~(31ull << (5 * ki))) | ((unsigned long long)e_of[d] << (5 * ki));
        loop_join();
    }
    wave_sync_mem();
    st.min_k = min_k; st.max_k = max_k; st.n_ent = n_ent; st.run_mask = run_mask; st.found_mask = found_mask; st.ent[0] = ent[0]; st.ent[1] = ent[1];
    if (bound_out) *bound_out = freq_bound;
}

// ---- phase 2: wrap_around_DP of every candidate ------------------------------------------------------------------------
// Candidates with units of at most 16 bases (most windows are microsatellite-sized, and a row of such a DP uses 16
// lanes of 64) wait for each other: up to four DISTINCT ones share a forward pass.  The others go one by one.
DEVINL void k2_range_dps(K2Ctx &c, int qs, int qe, const RangeP1 &st)
{
    const int n_ent = st.n_ent, min_k = st.min_k;
    const unsigned found_mask = st.found_mask;
    const int *pmeta = (const int *)(c.sc + c.y.pool_meta);
    const bool can_batch = dp_batch_fits(c, qe - qs + 1);
    int np = 0; unsigned pend = 0u, pU = 0u;                          // waiting entries and their unit lengths, 5 bits each
    unsigned key0 = 0u, key1 = 0u, key2 = 0u, key3 = 0u;
    for (int e = 0; e <= n_ent; e++) {
        bool flush = e == n_ent;                                       // the last turn only flushes
        RR t; rr_clear(t);
        int U = 0; unsigned key = 0u; bool small = false, waits = false;
        if (e < n_ent) {
            U = uni(pmeta[4 * e]);
            t.period = U; t.kmer = uni(pmeta[4 * e + 1]);
            small = can_batch && U <= 16;
            if (!((found_mask >> (t.kmer - min_k)) & 1u)) {
                // the last walk of this k failed: find_tandem_repeat_sub drops whatever the k found (the found flag is
                // that of the last attempt, SURVEY H4), so the alignment of this candidate is never looked at
                RR z; rr_clear(z); pool_store(c, e, z);
                wc_add(c.wc, CNT_MEMO_HITS, 1);
                wc_add(c.wc, CNT_MEMO_CELLS, 2ll * (long long)(qe - qs + 1) * (long long)U);
            }
            else if (!small) { dp_two_params(c, qs, qe, t, K2_NSLOT_FIXED + e); pool_store(c, e, t); }
            else if (memo_lookup(c, qs, qe, slot_unit(c, K2_NSLOT_FIXED + e), U, t)) pool_store(c, e, t);
            else {
                key = unit_key16(slot_unit(c, K2_NSLOT_FIXED + e), U);
                const bool dup = (np > 0 && ((pU >> 0) & 31u) == (unsigned)U && key0 == key) || (np > 1 && ((pU >> 5) & 31u) == (unsigned)U && key1 == key) ||
                                 (np > 2 && ((pU >> 10) & 31u) == (unsigned)U && key2 == key);
                waits = true;
                if (dup) flush = true;                                 // the same unit is waiting: align the waiting ones, then the memo answers
            }
        }
        if (flush || (waits && np == 4)) {
            if (np == 1) {
                const int e1 = (int)(pend & 31u);
                RR t1; rr_clear(t1); t1.period = (int)(pU & 31u); t1.kmer = uni(pmeta[4 * e1 + 1]);
                dp_two_params(c, qs, qe, t1, K2_NSLOT_FIXED + e1); pool_store(c, e1, t1);
            } else if (np > 1) dp_two_params_batch(c, qs, qe, np, pend);
            np = 0; pend = 0u; pU = 0u;
        }
        if (waits) {
            if (flush && memo_lookup(c, qs, qe, slot_unit(c, K2_NSLOT_FIXED + e), U, t)) pool_store(c, e, t);   // it was the duplicate
            else {
                pend |= (unsigned)e << (5 * np); pU |= (unsigned)U << (5 * np);
                if (np == 0) key0 = key; else if (np == 1) key1 = key; else if (np == 2) key2 = key; else key3 = key;
                np++;
                if (np == 4) { dp_two_params_batch(c, qs, qe, np, pend); np = 0; pend = 0u; pU = 0u; }
            }
        }
        loop_join();
    }
    (void)key3;
    wave_sync_mem();
}

// ---- phase 3: per k, in the reference's order, the selection among the two directions (search_De_Bruijn_graph :556-571),
// find_tandem_repeat_sub's checks and revision (handle_one_read.c:84-99), and the comparison over k (:136-146) ----------
// One k of phase 3 up to the revision: the selection among the two directions and find_tandem_repeat_sub's checks.  `cur` =
// the k's record so far (cleared if the k yields none), k_slot = the pool slot of its unit (-1: none); true = the revision
// (handle_one_read.c:95-97) is due.  copy: the unit goes to slot 1 (where revise() works); the staged mode loads it there itself.
DEVINL bool k2_select_k(K2Ctx &c, int qs, int qe, const RangeP1 &st, int k, RR &cur, int &k_slot, bool copy)
{
    const K2Args &a = *c.a;
    const int ki = k - st.min_k;
    rr_clear(cur);
    float k_ratio = -1.0f;
    k_slot = -1;
    for (int d = 0; d < 2; d++) {                                 // search_De_Bruijn_graph :556-571
        const int e = (int)((st.ent[d] >> (5 * ki)) & 31ull);
        if (e == 31) continue;
        RR t; pool_load(c, e, t);
        const float q = rr_ratio(t);
        if (k_ratio < q && a.min_match_ratio <= q && MTRC_MIN_NUM_FREQ_UNIT < t.copies &&
            MTRC_MIN_PERIOD <= t.period && t.period < MTRC_MAX_PERIOD) { k_ratio = q; cur = t; k_slot = K2_NSLOT_FIXED + e; }
    }
    if (copy && k_slot >= 0) slot_copy(c, 1, k_slot);
    trace_ev(c, 2, qs, qe, k, (int)((st.found_mask >> ki) & 1u), 0, cur.period, cur.rep_start, cur.rep_end, cur.repeat_len, cur.copies, cur.mat, cur.mis, cur.ins, cur.del);
    // find_tandem_repeat_sub (handle_one_read.c:77-100)
    if (!((st.found_mask >> ki) & 1u)) rr_clear(cur);
    else if ((long long)cur.period * (long long)(qe - qs + 1) > mtr_dev_wrap_dp_size) rr_clear(cur);
    else if (cur.period == 0) rr_clear(cur);
    else {
        const int coverage = cur.repeat_len / cur.period;
        return 5 <= coverage && coverage <= 20 && 5 < cur.period;
    }
    return false;
}
// the comparison over k (handle_one_read.c:136-146)
DEVINL bool k2_better(const K2Args &a, float best_ratio, const RR &cur)
{
    const float q = rr_ratio(cur);
    return best_ratio < q && a.min_match_ratio <= q && MTRC_MIN_NUM_FREQ_UNIT < cur.copies && MTRC_MIN_PERIOD <= cur.period;
}
DEVINL bool k2_qualifies(const RR &best) { return best.repeat_len > 0 && best.rep_start + MTRC_MIN_PERIOD * MTRC_MIN_NUM_FREQ_UNIT < best.rep_end; }

DEVINL bool k2_range_select(K2Ctx &c, int qs, int qe, const RangeP1 &st, RR &best)
{
    const K2Args &a = *c.a;
    rr_clear(best);
    float best_ratio = -1.0f;
    c.rmemo_n = 0;
    for (int k = st.min_k; k <= st.max_k; k++) {
        if (!((st.run_mask >> (k - st.min_k)) & 1u)) continue;
        RR cur; int k_slot;
        if (k2_select_k(c, qs, qe, st, k, cur, k_slot, true)) revise(c, cur);
        if (k2_better(a, best_ratio, cur)) { best_ratio = rr_ratio(cur); best = cur; slot_copy(c, 0, 1); }
        loop_join();
    }
    return k2_qualifies(best);
}

DEVINL bool k2_range(K2Ctx &c, int qs, int qe, int w, RR &best)
{
    RangeP1 st;
    k2_range_walks(c, qs, qe, w, st);
    k2_range_dps(c, qs, qe, st);
    return k2_range_select(c, qs, qe, st, best);
}

// remove_redundant_ranges_from_directional_index (handle_one_read.c:178-188): ranges after t that lie inside the repeat
DEVINL void prune_ranges(const int32_t *rs, int32_t *re, int t, int nr, int rep_start, int rep_end)
{
    const int lane = lane_id();
    for (int base = t + 1; base < nr; base += 64) {
        int u = base + lane;
        if (u < nr) {
            int s2 = rs[u], e2 = re[u];
            if (s2 >= rep_start && s2 < rep_end && e2 >= 0 && e2 < rep_end) re[u] = -1;
        }
    }
    wave_sync_mem();
}

// handle_one_TR's range loop (handle_one_read.c:227-246)
DEVINL void k2_read(K2Ctx &c)
{
    const K2Args &a = *c.a;
    const int lane = lane_id();
    const int rd = c.rd;
    const int nr = uni(a.r_count[rd]);
    const int64_t off = uni64(a.r_off[rd]);
    const int32_t *rs = a.r_start + off; int32_t *re = a.r_end + off; const int32_t *rw = a.r_w + off;
    int nrec = 0;
    c.memo_n = 0; c.memo_qs = c.memo_qe = -1; c.memo_U = 0;
    for (int t = 0; t < nr; t++) {
        const int qs = uni(rs[t]), qe = uni(re[t]), w = uni(rw[t]);   // loads are "divergent" to the compiler
        if (qe < 0) continue;                                            // pruned by an earlier repeat
        RR best;
        const bool rec = k2_range(c, qs, qe, w, best);
        wc_add(c.wc, CNT_RANGES_EXEC, 1);
        if (rec) {
            emit_record(c, best, nrec); nrec++;
            trace_ev(c, 6, best.rep_start, best.rep_end, best.repeat_len, best.period, best.copies, best.mat, best.mis, best.ins, best.del, best.kmer, best.G, best.MM, best.D, trace_on(c, 6) ? unit_hash(slot_unit(c, 0), best.period) : 0);
            prune_ranges(rs, re, t, nr, best.rep_start, best.rep_end);
        }
        loop_join();
    }
    if (lane == 0) a.rec_count[rd] = nrec;
    wc_add(c.wc, CNT_RECORDS, nrec);
}

// The per-read kernel.  A wavefront takes a read from the queue, finds its candidate ranges (k1_read, the
// window histograms borrow the LDS of the k-mer table) and then runs the unit search over them (k2_read).
template <bool MANHATTAN>
__global__ __launch_bounds__(64, MTR_WAVES_PER_SIMD) void mtr_k_reads(K1Args a1, K2Args a)
{
    // one LDS arena per wave: k-mer table keys (+ counts), seed list, 4x64 staging rows; the range phase of a
    // read uses all of it for its window difference fields
    __shared__ __attribute__((aligned(16))) int s_arena[MTR_ARENA_INTS];
    __shared__ unsigned long long s_cnt[CNT_N];
    static_assert(MTR_ARENA_INTS == K2_TAB_CAP + MTRC_MAX_SEEDS + 4 + 4 * 64, "arena layout");
    int *s_keys = s_arena, *s_seeds = s_arena + K2_TAB_CAP, *s_stage = s_seeds + MTRC_MAX_SEEDS + 4;
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    K2Ctx c;
    c.a = &a;
    c.wc = s_cnt;
    c.sc = a.scratch + (size_t)blockIdx.x * a.scratch_per_wave;
    c.y = k2_layout(a.Lmax);
    c.lds_keys = (lds_int *)s_keys; c.seeds = (lds_int *)s_seeds; c.stage = (lds_int *)s_stage;
    c.ties = (int *)(c.sc + c.y.ties); c.fresh = c.ties + MTRC_MAX_TIEBREAKS;
    for (;;) {
        const int t = next_work_item(a.work_counter);
        if (t >= a.b.n_reads) break;                   // every wave reaches this exit
        c.rd = uni(a.b.order[t]);
        c.L = uni(a.b.lens[c.rd]);
        c.pk = a.b.packed + uni64(a.b.woff[c.rd]);
        const unsigned long long t_read = clk();
#ifdef MTR_PROFILE
        const unsigned long long rt_read = __builtin_amdgcn_s_memrealtime();       // 100 MHz constant clock
#endif
        k1_read<MANHATTAN>(a1, c.rd, c.sc, (lds_u8 *)s_arena, MTR_ARENA_INTS * 4, s_cnt);
        wave_sync_mem();
        k2_read(c);
        wc_time(s_cnt, CYC_TOTAL, t_read);
#ifdef MTR_PROFILE
        wc_add(s_cnt, CNT_RESERVED15, (long long)(__builtin_amdgcn_s_memrealtime() - rt_read));
#endif
        // per-read cost record (trace type 7, units of 1024 cycles): total, DP fwd, DP tb, rev fwd, rev tb, tables, walks
        trace_ev(c, 7, (int)(s_cnt[CYC_TOTAL] >> 10), (int)(s_cnt[CYC_DP_FWD] >> 10), (int)(s_cnt[CYC_DP_TB] >> 10),
                 (int)(s_cnt[CYC_DP_FWD_REV] >> 10), (int)(s_cnt[CYC_DP_TB_REV] >> 10), (int)(s_cnt[CYC_TAB_BUILD] >> 10),
                 (int)(s_cnt[CYC_WALK] >> 10), (int)s_cnt[CNT_DP_CALLS], (int)(s_cnt[CNT_DP_CELLS] >> 10), (int)(s_cnt[CNT_LOOKUPS] >> 10),
                 (int)s_cnt[CNT_TABLES], (int)s_cnt[CNT_RANGES_EXEC], (int)s_cnt[CNT_TB_STEPS], c.L);
        if (a.trace_cap > 0) wc_flush(s_cnt, a.counters);      // the cost records above are per read
        loop_join();
    }
    // once per wavefront: the counters share a few cache lines, and atomics on one line complete one after the other chip-wide
    // (11 ns each, tests/dev/atomic_rate.hip) - a flush per read was up to 0.5 M of them per launch
    wc_flush(s_cnt, a.counters);
}

// The unit phase alone, one wavefront per read, over ranges a range kernel has left in r_start / r_end / r_w: the second
// half of the file-order mode (mtr_upload_batch_in_file), whose range phase (mtr_k1_ranges with the stale tails) is a
// kernel of its own so that the per-read kernel above stays what it is.
__global__ __launch_bounds__(64, MTR_WAVES_PER_SIMD) void mtr_k_units(K2Args a)
{
    __shared__ __attribute__((aligned(16))) int s_arena[MTR_ARENA_INTS];
    __shared__ unsigned long long s_cnt[CNT_N];
    int *s_keys = s_arena, *s_seeds = s_arena + K2_TAB_CAP, *s_stage = s_seeds + MTRC_MAX_SEEDS + 4;
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    K2Ctx c;
    c.a = &a;
    c.wc = s_cnt;
    c.sc = a.scratch + (size_t)blockIdx.x * a.scratch_per_wave;
    c.y = k2_layout(a.Lmax);
    c.lds_keys = (lds_int *)s_keys; c.seeds = (lds_int *)s_seeds; c.stage = (lds_int *)s_stage;
    c.ties = (int *)(c.sc + c.y.ties); c.fresh = c.ties + MTRC_MAX_TIEBREAKS;
    for (;;) {
        const int t = next_work_item(a.work_counter);
        if (t >= a.b.n_reads) break;                   // every wave reaches this exit
        c.rd = uni(a.b.order[t]);
        c.L = uni(a.b.lens[c.rd]);
        c.pk = a.b.packed + uni64(a.b.woff[c.rd]);
        const unsigned long long t_read = clk();
        k2_read(c);
        wc_time(s_cnt, CYC_TOTAL, t_read);
        loop_join();
    }
    wc_flush(s_cnt, a.counters);
}

// ---------------------------------------------------------------------------------------------------------
// The replay of the reference's sequential range loop (staged chain, k3_staged.hip.inc).  A range's unit search depends on nothing
// but the read and the range; what the reference's loop adds is only that a reported repeat removes later ranges that lie inside it
// (handle_one_read.c:178-188, :242-243).  The chain searches ALL ranges as independent work items and parks the candidate record
// of a range that qualifies; mtr_k_replay walks each read's ranges in order, skips the ones an accepted record has removed, and
// moves the surviving candidates to the read's record slots - the same records in the same order.
// ---------------------------------------------------------------------------------------------------------
struct SplitArgs {
    const int64_t *item_off;       // read -> index of its first range among all ranges of the batch
    DevRecord *cand;               // the parked records
    int32_t *cand_flag;            // per range: 1 + index into cand of the range's record, 0 = none
};

// The range loop of handle_one_read.c:227-246 over ranges whose searches are done, 64 ranges at a time: lane l holds range base + l - its end (negative: removed
// by an accepted repeat, :178-188) and its flag -, one round trip per 64 ranges; the loop's order only matters at a range that carries a record (a few per read),
// where the pruning (prune_ranges: global memory) runs and the lanes behind it load their ends again.  Before: one dependent load per range and read - ~216 round
// trips per 2 kb read on a wavefront that did nothing else (mtr_k_replay + mtr_k_pass_mark: 7.6 G of the launch's wavefront-cycles for 23 M instructions).
// flag_of(t) = range t's flag (called per lane); on_record(t, flag) is called - by the whole wavefront, t uniform - for every reached range with flag != 0
// and returns false to stop the read's loop.
// Returns the number of ranges the loop reached.
template <typename L, typename F>
DEVINL long long replay_ranges(int32_t *re, int nr, L &&flag_of, F &&on_record)
{
    const int lane = lane_id();
    long long executed = 0;
    for (int base = 0; base < nr; base += 64) {
        const int t = base + lane;
        const bool valid = t < nr;
        int e_l = valid ? re[t] : -1;
        const int f_l = valid ? flag_of(t) : 0;              // (per lane)
        int pos = 0;
        while (pos < 64) {
            const unsigned long long behind = ~0ull << pos;
            const unsigned long long alive = __ballot(valid && e_l >= 0) & behind;
            const unsigned long long marked = __ballot(valid && e_l >= 0 && f_l != 0) & behind;
            if (marked == 0ull) { executed += __popcll(alive); break; }
            const int j = first_lane(marked);
            executed += __popcll(alive & ((1ull << j) - 1ull)) + 1;
            if (!on_record(base + j, lane_val(f_l, j))) return executed;
            if (valid) e_l = re[t];                              // (what the record removed; on_record's pruning ended with a fence)
            pos = j + 1;
            loop_join();
        }
        loop_join();
    }
    return executed;
}

// one wavefront per read: the reference's range loop with the searches already done
__global__ __launch_bounds__(64) void mtr_k_replay(K2Args a, SplitArgs s)
{
    const int lane = lane_id();
    // A chain that outgrew a buffer left its flags half written - after a full list of the dead-range screen the walks did not run, and in one
    // pass nothing else writes a kept range's flag: what the buffer held before would be taken for an index into cand.  The host reruns the batch.
    if (uni(*(volatile int32_t *)a.status) == DEV_ERR_STAGED_OVERFLOW) return;
    for (int rd = blockIdx.x; rd < a.b.n_reads; rd += gridDim.x) {
        int hv = 0; long long ho = 0;
        if (lane == 0) { hv = a.r_count[rd]; ho = a.r_off[rd]; } else if (lane == 1) ho = s.item_off[rd];
        const int nr = lane_val(hv, 0);
        const int64_t off = lane_val64(ho, 0), first = lane_val64(ho, 1);
        const int32_t *rs = a.r_start + off; int32_t *re = a.r_end + off;
        int nrec = 0;
        bool sent_back = false;
        const int32_t *flags = s.cand_flag + first;
        const long long executed = replay_ranges(re, nr, [&](int t) -> int { return flags[t]; }, [&](int t, int flag) -> bool {
            if (flag < 0) {
                // (two passes, k3_staged.hip.inc) the loop reaches a range that neither pass searched: this read goes through the per-read
                // kernel, by the path of the reads that found more records than they have slots
                sent_back = true;
                return false;
            }
            const DevRecord *src = s.cand + (flag - 1);
            if (nrec < a.max_rec_per_read) {                  // else only counted: the host reruns the read with more room
                const int64_t base = a.rec_base ? uni64(a.rec_base[rd]) : (int64_t)rd * (int64_t)a.max_rec_per_read;
                const uint4 *sp = (const uint4 *)src;
                uint4 *dp = (uint4 *)(a.records + base + nrec);
                for (int q = lane; q < (int)(sizeof(DevRecord) / 16); q += 64) dp[q] = sp[q];
            }
            nrec++;
            const int rep_start = uni(src->f[0]), rep_end = uni(src->f[1]);
            prune_ranges(rs, re, t, nr, rep_start, rep_end);
            return true;
        });
        if (lane == 0) {
            a.rec_count[rd] = sent_back ? 4 * a.max_rec_per_read + 4096 : nrec;
            if (sent_back) atomicAdd(&a.counters[CNT_SPARE53], 1ull);
            else {
                atomicAdd(&a.counters[CNT_RECORDS], (unsigned long long)nrec);
                atomicAdd(&a.counters[CNT_RANGES_EXEC], (unsigned long long)executed);
            }
        }
    }
}

// -a: the alignment of every reported repeat (A9).  Same recurrence and traceback as wrap_around_DP_sub, on
// org[rep_start-1+i], i = 1..rep_end-rep_start+1, with the record's own scores; the path comes back as one byte per
// column (the host turns it into the three text rows, 50 columns per block).
__global__ __launch_bounds__(64) void mtr_k_align(AlignArgs a)
{
    __shared__ unsigned long long s_cnt[CNT_N];
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    uint8_t *sc = a.scratch + (size_t)blockIdx.x * a.scratch_per_wave;
    for (;;) {
        const int t = next_work_item(a.work_counter);
        if (t >= a.n_tasks) break;
        const int rd = uni(a.read_idx[t]);
        const uint32_t *pk = a.b.packed + uni64(a.b.woff[rd]);
        const int rs = uni(a.rep_start[t]), re = uni(a.rep_end[t]);
        const int uo = uni(a.unit_off[t]), U = uni(a.unit_off[t + 1]) - uo;
        const int64_t o0 = uni64(a.ops_off[t]), o1 = uni64(a.ops_off[t + 1]);
        TbOps out; out.ops = a.ops + o0; out.cap = (int)(o1 - o0); out.n = 0; out.overflow = 0;
        DpRes o;
        const bool ok = dp_wrap(pk, rs - 1, re - rs + 1, a.units + uo, U, uni(a.gain[t]), uni(a.mism[t]), uni(a.indel[t]), sc, a.cells_cap,
                                2, nullptr, nullptr, nullptr, o, s_cnt, a.dp16_max_rows, &out);
        if (!ok) set_status(a.status, DEV_ERR_DP_TOO_LARGE);
        if (out.overflow) set_status(a.status, DEV_ERR_RECORD_OVERFLOW);
        if (lane_id() == 0) { a.ops_len[t] = out.n; a.ends[2 * t] = out.n > 0 ? o.end_i : 0; a.ends[2 * t + 1] = o.end_j; }
        loop_join();
    }
}

// test kernel: wrap_around_DP_sub for a list of (read, window, unit, scores) tasks
__global__ __launch_bounds__(64) void mtr_k_dp_test(DpTestArgs a)
{
    __shared__ unsigned long long s_cnt[CNT_N];
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    uint8_t *sc = a.scratch + (size_t)blockIdx.x * a.scratch_per_wave;
    for (;;) {
        const int t = next_work_item(a.work_counter);
        if (t >= a.n_tasks) break;
        int rd = a.read_idx[t];
        const uint32_t *pk = a.b.packed + a.b.woff[rd];
        int qs = a.qs[t], qe = a.qe[t];
        int U = a.unit_off[t + 1] - a.unit_off[t];
        DpRes o;
        bool ok = dp_wrap(pk, qs, qe - qs + 1, a.units + a.unit_off[t], U, a.gain[t], a.mism[t], a.indel[t], sc, a.cells_cap, 0, nullptr, nullptr, nullptr, o, s_cnt, a.dp16_max_rows);
        if (!ok) set_status(a.status, DEV_ERR_DP_TOO_LARGE);
        if (lane_id() == 0) {
            int32_t *r = a.out8 + (size_t)t * 8;
            r[0] = qs + o.stop_i + 1; r[1] = qs + o.end_i; r[2] = o.end_i - o.stop_i; r[3] = U > 0 ? o.scanned / U : 0;
            r[4] = o.mat; r[5] = o.mis; r[6] = o.ins; r[7] = o.del;
        }
        wc_flush(s_cnt, a.counters);
        loop_join();
    }
}
