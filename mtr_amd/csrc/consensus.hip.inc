// consensus.hip.inc — the oriented windows of genotype rows out of the resident batch (mtr_extract_windows_device) and the allele consensus
// over them (mtr_allele_consensus_device).  The definition is include/mtr_hip.h's ("allele consensus"); the band, the cell, the schedule, the
// vote walk and the emission of a position are banded_align.h, shared with the host.  Every result is an exact integer: the votes are integer
// atomic adds, whose order reaches no sum.
//   mtr_k_win_len        one lane per row: its read inside the batch, its window inside the read (the smallest bad row is left in the state), its length
//   mtr_k_win_gather     one wavefront per row: 64 bases a turn out of the packed 2-bit words, reverse-complemented for orientation 1, one byte per lane
//   mtr_k_cons_check     one lane per row / locus: the rows ascending by (read, locus), the two offset columns, the zygosities
//   mtr_k_cons_members   one lane per support entry: its row by bisection over (read, locus); the allele column 0 .. 0 1 .. 1 within a locus
//   mtr_k_cons_alleles   one lane per allele: its segment, its backbone entry, the length of its vote table
//   mtr_k_cons_tasks     one lane per support entry: a member that is not the backbone becomes a task of its band bucket, or is counted as skipped
//   mtr_k_cons_align<CPL> THE HOT PATH, one alignment per wavefront: the fill by anti-diagonals (banded_align.h), lane t holding the pairs
//                        t * CPL .. t * CPL + CPL - 1 - one DPP wavefront shift per step brings the one neighbour value - the directions packed
//                        16 steps a dword into the wavefront's scratch (256 contiguous bytes per store), then the vote walk by lane 0
//   mtr_k_cons_emit<W>   one workgroup per allele: per position its symbols (ba_emit), a scan, and - W = 1 - the writes; W = 0 gives the lengths
#pragma once
#include "device_util.hip.inc"
#include "banded_align.h"

#define CO_BLOCK 256
#define CO_BAD 8                    // uint64 each, ~0: none.  0 rows out of order, 1 win_off, 2 support_off / zygosity, 3 entry without a row, 4 allele column, 5 a window (extract)
#define CO_STATE 4                  // uint32: tasks of bucket 0, of bucket 1, the longest n + m of bucket 0, of bucket 1
#define CO_MAX_GRID (1 << 16)

struct ConsArgs {
    const int32_t *row_read, *row_locus; int64_t R;
    const int64_t *win_off; const uint8_t *win_bases; int64_t n_bases;
    const int64_t *support_off; const int32_t *sup_read; const uint8_t *sup_allele, *zygosity; int64_t S; int32_t n_loci, band_extra;
    int32_t *ent_row;                                                   // [S]
    int32_t *bb_ent, *bb_row, *bb_read, *bb_len, *members, *aligned, *skipped, *tab_len, *cons_len;      // [2 * n_loci] each
    int64_t *tab_off, *cons_off;                                        // [2 * n_loci + 1] each
    int32_t *tab;                                                       // [tab_off[2 * n_loci] * BA_TAB], zeroed per call
    int4 *tasks;                                                        // bucket b's at tasks + b * S: allele, member row, backbone row
    unsigned *state; unsigned long long *bad;
    uint8_t *bases; int32_t *votes;                                     // the caller's
};

DEVINL unsigned long long cons_key(int32_t read, int32_t locus) { return ((unsigned long long)(uint32_t)read << 32) | (uint32_t)locus; }
// the locus of support entry e: the last l with support_off[l] <= e (loci without support own no entry)
DEVINL int32_t cons_locus(const ConsArgs &a, int64_t e)
{
    int32_t lo = 0, hi = a.n_loci - 1;
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (a.support_off[mid] <= e) lo = mid; else hi = mid - 1; }
    return lo;
}
// the row of (read, locus) by bisection over the rows' ascending keys, -1 without one
DEVINL int32_t cons_row_of(const ConsArgs &a, unsigned long long key)
{
    int64_t lo = 0, hi = a.R;                                           // the first row whose key is not below the entry's
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (cons_key(a.row_read[mid], a.row_locus[mid]) < key) lo = mid + 1; else hi = mid; }
    return lo < a.R && cons_key(a.row_read[lo], a.row_locus[lo]) == key ? (int32_t)lo : -1;
}
// the segment [lo, hi) of allele a of locus l within the locus' entries
DEVINL void cons_segment(const ConsArgs &a, int32_t l, int al, int64_t &lo, int64_t &hi)
{
    lo = a.support_off[l]; hi = a.support_off[l + 1];
    int64_t x = lo, y = hi;                                             // the first entry of allele 1
    while (x < y) { const int64_t mid = (x + y) >> 1; if (a.sup_allele[mid] == 0) x = mid + 1; else y = mid; }
    if (al == 0) hi = x; else lo = x;
}
DEVINL bool cons_allele_exists(int z, int al) { return z == 2 || (z == 1 && al == 0); }

// ---- windows --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CO_BLOCK) void mtr_k_win_len(const int32_t *row_read, const int32_t *window, int64_t R, const int32_t *lens, int32_t n_reads, int32_t *len,
                                                          unsigned long long *bad)
{
    const int64_t r = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int32_t rd = row_read[r], lo = window[2 * r], hi = window[2 * r + 1];
    int32_t n = 0;
    if (rd < 0 || rd >= n_reads || lo < 0 || hi < lo || hi > lens[rd]) atomicMin(&bad[5], (unsigned long long)r);
    else n = hi - lo;
    len[r] = n;
}

__global__ __launch_bounds__(64) void mtr_k_win_gather(const int32_t *row_read, const uint8_t *orientation, const int32_t *window, int64_t R, const uint32_t *packed,
                                                       const int64_t *woff, const int64_t *win_off, uint8_t *dst)
{
    const int lane = lane_id();
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        const uint32_t *pk = packed + woff[row_read[r]];
        const int32_t lo = window[2 * r], hi = window[2 * r + 1];
        const bool rc = orientation[r] == 1;
        uint8_t *out = dst + win_off[r];
        for (int32_t t = lane; t < hi - lo; t += 64) out[t] = (uint8_t)(rc ? 3 - base_at(pk, hi - 1 - t) : base_at(pk, lo + t));
    }
}

// ---- the consensus' lists ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CO_BLOCK) void mtr_k_cons_check(ConsArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
    if (x < a.R) {
        if (x > 0 && !(cons_key(a.row_read[x - 1], a.row_locus[x - 1]) < cons_key(a.row_read[x], a.row_locus[x]))) atomicMin(&a.bad[0], (unsigned long long)x);
        if (a.row_read[x] < 0 || a.row_locus[x] < 0) atomicMin(&a.bad[0], (unsigned long long)x);
        const int64_t o0 = a.win_off[x], o1 = a.win_off[x + 1];
        if (o0 < 0 || o1 < o0 || o1 > a.n_bases || o1 - o0 > (int64_t)(1 << 30) || (x == 0 && o0 != 0)) atomicMin(&a.bad[1], (unsigned long long)x);
    }
    if (x < a.n_loci) {
        const int64_t o0 = a.support_off[x], o1 = a.support_off[x + 1];
        if (o0 < 0 || o1 < o0 || o1 > a.S || (x == 0 && o0 != 0) || (x == a.n_loci - 1 && o1 != a.S) || a.zygosity[x] > 2) atomicMin(&a.bad[2], (unsigned long long)x);
    }
}

__global__ __launch_bounds__(CO_BLOCK) void mtr_k_cons_members(ConsArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
    if (e >= a.S) return;
    const int32_t l = cons_locus(a, e);
    const int32_t row = cons_row_of(a, cons_key(a.sup_read[e], l));
    a.ent_row[e] = row;
    if (row < 0) atomicMin(&a.bad[3], (unsigned long long)e);
    if (a.sup_allele[e] > 1 || (e > a.support_off[l] && a.sup_allele[e] < a.sup_allele[e - 1])) atomicMin(&a.bad[4], (unsigned long long)e);
}

__global__ __launch_bounds__(CO_BLOCK) void mtr_k_cons_alleles(ConsArgs a)
{
    const int64_t A = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
    if (A >= 2 * (int64_t)a.n_loci) return;
    const int32_t l = (int32_t)(A >> 1); const int al = (int)(A & 1);
    int64_t lo, hi;
    cons_segment(a, l, al, lo, hi);
    const int64_t n = cons_allele_exists(a.zygosity[l], al) ? hi - lo : 0;
    int32_t ent = -1, row = -1, rd = -1, len = 0;
    if (n > 0) {
        ent = (int32_t)(lo + (n - 1) / 2); row = a.ent_row[ent]; rd = a.sup_read[ent];
        len = (int32_t)(a.win_off[row + 1] - a.win_off[row]);
    }
    a.bb_ent[A] = ent; a.bb_row[A] = row; a.bb_read[A] = rd; a.bb_len[A] = len; a.members[A] = (int32_t)n; a.tab_len[A] = n > 0 ? len + 1 : 0;
}

__global__ __launch_bounds__(CO_BLOCK) void mtr_k_cons_tasks(ConsArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
    if (e >= a.S) return;
    const int32_t l = cons_locus(a, e); const int al = a.sup_allele[e];
    if (!cons_allele_exists(a.zygosity[l], al)) return;
    const int64_t A = 2 * (int64_t)l + al;
    if (a.bb_ent[A] == (int32_t)e) return;
    const int32_t row = a.ent_row[e], bb = a.bb_row[A];
    const int64_t n = a.win_off[row + 1] - a.win_off[row], m = a.bb_len[A];
    if (ba_skipped(n, m, a.band_extra)) { atomicAdd(&a.skipped[A], 1); return; }
    const int b = ba_width(ba_band((int32_t)n, (int32_t)m, a.band_extra)) <= 128 ? 0 : 1;
    const unsigned slot = atomicAdd(&a.state[b], 1u);
    if ((int64_t)slot < a.S) a.tasks[(int64_t)b * a.S + slot] = make_int4((int)A, row, bb, 0);
    atomicMax(&a.state[2 + b], (unsigned)(n + m));
    atomicAdd(&a.aligned[A], 1);
}

// value of lane + 1 (lane 63 receives `last`): wave_shl:1
DEVINL int shift_down1(int v, int last)
{
    return __builtin_amdgcn_update_dpp(last, v, 0x130, 0xf, 0xf, false);
}

// ---- the alignment ------------------------------------------------------------------------------------------------------------------------------
// scratch: words_per_wave dwords per wavefront of the grid, enough for the bucket's longest task (ba_dir_words)
template <int CPL>
__global__ __launch_bounds__(64) void mtr_k_cons_align(ConsArgs a, int bucket, unsigned n_tasks, uint32_t *scratch, int64_t words_per_wave)
{
    const int lane = lane_id();
    uint32_t *dirs = scratch + (int64_t)blockIdx.x * words_per_wave;
    for (unsigned t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const int4 task = a.tasks[(int64_t)bucket * a.S + t];
        const int A = uni(task.x), row = uni(task.y), bb = uni(task.z);
        const int64_t wo = uni64(a.win_off[row]), bo = uni64(a.win_off[bb]);
        const int32_t n = uni((int)(a.win_off[row + 1] - wo)), m = uni((int)(a.win_off[bb + 1] - bo));
        const uint8_t *W = a.win_bases + wo, *B = a.win_bases + bo;
        const BaBand band = ba_band(n, m, a.band_extra);
        if (ba_dir_words(n, m, CPL) <= words_per_wave && ba_width(band) <= 128 * CPL) {        // (the host sized both: nothing is stored past them)
            int32_t E[CPL], O[CPL]; uint32_t acc[CPL];
#pragma unroll
            for (int k = 0; k < CPL; k++) { E[k] = O[k] = BA_INF; acc[k] = 0u; }
            for (int32_t s = 0; s <= n + m; s++) {
                const int sh = 2 * (s & 15);
                if (((s - band.dlo) & 1) == 0) {
                    const int32_t below = shift_up1(O[CPL - 1], BA_INF);
#pragma unroll
                    for (int k = 0; k < CPL; k++) {
                        int dir;
                        E[k] = ba_step_cell(s, 2 * (lane * CPL + k), n, m, band, E[k], O[k], k > 0 ? O[k > 0 ? k - 1 : 0] : below, W, B, dir);
                        acc[k] |= (uint32_t)dir << sh;
                    }
                } else {
                    const int32_t above = shift_down1(E[0], BA_INF);
#pragma unroll
                    for (int k = 0; k < CPL; k++) {
                        int dir;
                        O[k] = ba_step_cell(s, 2 * (lane * CPL + k) + 1, n, m, band, O[k], k + 1 < CPL ? E[k + 1 < CPL ? k + 1 : 0] : above, E[k], W, B, dir);
                        acc[k] |= (uint32_t)dir << sh;
                    }
                }
                if (sh == 30 || s == n + m) {
#pragma unroll
                    for (int k = 0; k < CPL; k++) { dirs[((int64_t)(s >> 4) * CPL + k) * 64 + lane] = acc[k]; acc[k] = 0u; }
                }
            }
            wave_sync_mem();
            if (lane == 0) {
                int32_t *tab = a.tab + a.tab_off[A] * BA_TAB;
                const int32_t dlo = band.dlo;
                ba_walk(n, m, W, [=](int32_t i, int32_t j) { return ba_dir_at(dirs, i, j, dlo, CPL); }, [=](int64_t x) { atomicAdd(tab + x, 1); });
            }
            wave_sync_mem();                                            // (the walk has read the directions before the next task's overwrite them)
        }
        loop_join();
    }
}

// ---- the emission ---------------------------------------------------------------------------------------------------------------------------------
template <int WRITE>
__global__ __launch_bounds__(CO_BLOCK) void mtr_k_cons_emit(ConsArgs a)
{
    __shared__ int32_t part[CO_BLOCK / 64];
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (int64_t A = blockIdx.x; A < 2 * (int64_t)a.n_loci; A += gridDim.x) {
        const int32_t row = a.bb_row[A], m = a.bb_len[A], N = 1 + a.aligned[A];
        int64_t before = 0;
        if (row >= 0) {
            const uint8_t *B = a.win_bases + a.win_off[row];
            const int32_t *tab = a.tab + a.tab_off[A] * BA_TAB;
            for (int32_t c = 0; c <= m; c += CO_BLOCK) {
                const int32_t j = c + tid;
                uint8_t sym[1 + BA_INS_SLOTS]; int32_t vt[1 + BA_INS_SLOTS];
                const int em = j <= m ? ba_emit(tab + (int64_t)j * BA_TAB, j, j >= 1 ? B[j - 1] : 0, N, sym, vt) : 0;
                const int has_base = em & 1, n_ins = em >> 1, cnt = has_base + n_ins;
                int inc = cnt;
                for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
                __syncthreads();
                if (lane == 63) part[wave] = inc;
                __syncthreads();
                int total = 0;
                for (int w = 0; w < CO_BLOCK / 64; w++) { const int s = part[w]; if (w < wave) inc += s; total += s; }
                if (WRITE) {
                    const int64_t at = a.cons_off[A] + before + inc - cnt;
#pragma unroll
                    for (int k = 0; k < 1 + BA_INS_SLOTS; k++)
                        if (k == 0 ? has_base : k <= n_ins) { const int64_t to = at + (k == 0 ? 0 : has_base + k - 1); a.bases[to] = sym[k]; a.votes[to] = vt[k]; }
                }
                before += total;
            }
        }
        if (!WRITE && tid == 0) a.cons_len[A] = (int32_t)before;
    }
}
