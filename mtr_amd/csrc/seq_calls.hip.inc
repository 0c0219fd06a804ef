// seq_calls.hip.inc — allele calls by sequence (mtr_call_alleles_sequence_device): per locus the saturated edit distance between every two
// supporting reads' oriented windows, and from those distances an exact one- or two-medoid split.  The definition is include/mtr_hip.h's
// ("sequence allele calls"); the distance's band and clamp, the pair index, the medoid keys and the partition are seq_calls.h, shared with the
// host; the cell and the anti-diagonal schedule are banded_align.h's.  Every result is an exact integer and none depends on the order in which
// the device worked: the only atomics hand out task slots, and a task carries the place of its result.
//   mtr_k_seq_check      one lane per row / locus: the rows ascending by (read, locus), the two offset columns
//   mtr_k_seq_members    one lane per support entry: its row by the consensus' bisection over (read, locus)
//   mtr_k_seq_loci       one lane per locus: skipped above SQ_MAX_MEMBERS members, else its S (S - 1) / 2 pairs (mtr_k_scan_offsets makes pair_off)
//   mtr_k_seq_tasks      one lane per pair: resolved at once - K + 1 by the length rule, n for an empty window - or a task of its band's bucket,
//                        the slots handed out one atomic per wavefront and bucket
//   mtr_k_seq_dist<ROWS, CPL>  THE HOT PATH, the banded fill without directions, nothing stored per cell, no scratch.  <4, 1>: FOUR alignments per
//                        wavefront, one per 16-lane DPP row, lane r of a row holding the pair of diagonals r (bands of up to 32 diagonals, K <=
//                        31 always): the neighbour values come by row shifts, BA_INF entering at the row's ends; the four tasks have lengths and
//                        parities of their own, a row that is done holds its values while the others finish.  <2, 1>: TWO per wavefront, one per
//                        half of 32 lanes (bands of up to 64 diagonals - K = 32, whose bands are 33 wide for lengths of equal parity), by wavefront
//                        shifts with BA_INF put at the halves' border.  <1, 1> and <1, 2>: one alignment per wavefront, one or two pairs per lane
//                        (bands of up to 128 and 256 diagonals), as mtr_k_cons_align
//   mtr_k_seq_split      one wavefront per locus: D out of the upper triangle into LDS as bytes (128 x 128), the lanes enumerate the medoids and
//                        the medoid pairs, each keeping its least key, a wavefront reduction, then the stable partition by ballots and the
//                        per-locus columns
#pragma once
#include "consensus.hip.inc"
#include "seq_calls.h"

#define SQ_BLOCK 256
#define SQ_STATE SQ_BUCKETS         // uint32: the tasks of the four buckets
#define SQ_MAX_GRID (1 << 16)
#define SQ_LDS (SQ_MAX_MEMBERS * SQ_MAX_MEMBERS)

struct SeqArgs {
    ConsArgs c;                                                         // the rows, the windows, the support lists; ent_row [S], bad, state
    const int32_t *value; SqParams prm;
    int32_t *npairs;                                                    // [n_loci]
    int64_t *pair_off; int64_t P;                                       // [n_loci + 1]
    int4 *tasks;                                                        // [2 P]: member row, member row, the pair's place (low, high).  Bucket 0 from tasks up, 1 from tasks + P - 1 down, 2 from tasks + P up, 3 from tasks + 2 P - 1 down
    uint8_t *dist;                                                      // [P]
    int32_t *o_value, *o_read, *o_dtm; uint8_t *o_allele;               // [S]
    uint8_t *o_zyg, *o_skipped; int32_t *o_call, *o_sup, *o_medoid; int64_t *o_cost;       // per locus
};

// value of the next lane of the same 16-lane row (the row's last lane receives `last`): row_shl:1
DEVINL int row_shift_down1(int v, int last)
{
    return __builtin_amdgcn_update_dpp(last, v, 0x101, 0xf, 0xf, false);
}
DEVINL uint32_t wave_min_u32(uint32_t v)
{
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64); v = o < v ? o : v; }
    return v;
}

// ---- the lists ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SQ_BLOCK) void mtr_k_seq_check(SeqArgs a)
{
    const ConsArgs &c = a.c;
    const int64_t x = (int64_t)blockIdx.x * SQ_BLOCK + threadIdx.x;
    if (x < c.R) {
        if (x > 0 && !(cons_key(c.row_read[x - 1], c.row_locus[x - 1]) < cons_key(c.row_read[x], c.row_locus[x]))) atomicMin(&c.bad[0], (unsigned long long)x);
        if (c.row_read[x] < 0 || c.row_locus[x] < 0) atomicMin(&c.bad[0], (unsigned long long)x);
        const int64_t o0 = c.win_off[x], o1 = c.win_off[x + 1];
        if (o0 < 0 || o1 < o0 || o1 > c.n_bases || o1 - o0 > (int64_t)(1 << 30) || (x == 0 && o0 != 0)) atomicMin(&c.bad[1], (unsigned long long)x);
    }
    if (x < c.n_loci) {
        const int64_t o0 = c.support_off[x], o1 = c.support_off[x + 1];
        if (o0 < 0 || o1 < o0 || o1 > c.S || (x == 0 && o0 != 0) || (x == c.n_loci - 1 && o1 != c.S)) atomicMin(&c.bad[2], (unsigned long long)x);
    }
}

__global__ __launch_bounds__(SQ_BLOCK) void mtr_k_seq_members(SeqArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * SQ_BLOCK + threadIdx.x;
    if (e >= a.c.S) return;
    const int32_t row = cons_row_of(a.c, cons_key(a.c.sup_read[e], cons_locus(a.c, e)));
    a.c.ent_row[e] = row;
    if (row < 0) atomicMin(&a.c.bad[3], (unsigned long long)e);
}

__global__ __launch_bounds__(SQ_BLOCK) void mtr_k_seq_loci(SeqArgs a)
{
    const int64_t l = (int64_t)blockIdx.x * SQ_BLOCK + threadIdx.x;
    if (l >= a.c.n_loci) return;
    const int64_t S = a.c.support_off[l + 1] - a.c.support_off[l];
    const bool skipped = S > SQ_MAX_MEMBERS;
    a.o_skipped[l] = skipped ? 1 : 0;
    a.npairs[l] = skipped ? 0 : (int32_t)sq_pairs(S);
}

__global__ __launch_bounds__(SQ_BLOCK) void mtr_k_seq_tasks(SeqArgs a)
{
    const ConsArgs &c = a.c;
    const int lane = lane_id();
    const int32_t K = a.prm.max_dist;
    for (int64_t first = (int64_t)blockIdx.x * SQ_BLOCK + (threadIdx.x & ~63u); first < a.P; first += (int64_t)gridDim.x * SQ_BLOCK) {    // (the same for a wavefront's lanes)
        const int64_t p = first + lane;
        int bucket = -1;
        int4 task = make_int4(0, 0, 0, 0);
        if (p < a.P) {
            int32_t lo = 0, hi = c.n_loci - 1;                              // the locus that owns place p: the last l with pair_off[l] <= p
            while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (a.pair_off[mid] <= p) lo = mid; else hi = mid - 1; }
            const int64_t e0 = c.support_off[lo];
            const int32_t S = (int32_t)(c.support_off[lo + 1] - e0);
            int32_t t, u;
            sq_pair_at(S, p - a.pair_off[lo], t, u);
            const int32_t rt = c.ent_row[e0 + t], ru = c.ent_row[e0 + u];
            const int64_t n = c.win_off[rt + 1] - c.win_off[rt], m = c.win_off[ru + 1] - c.win_off[ru];
            if (sq_far(n, m, K)) a.dist[p] = (uint8_t)(K + 1);
            else if (n == 0 || m == 0) a.dist[p] = (uint8_t)(n + m);        // (|n - m| <= K: the other window's length)
            else {
                bucket = sq_bucket(ba_width(sq_band((int32_t)n, (int32_t)m, K)));
                task = make_int4(rt, ru, (int)(uint32_t)p, (int)(uint32_t)((uint64_t)p >> 32));
            }
        }
        for (int b = 0; b < SQ_BUCKETS; b++) {
            const unsigned long long mask = __ballot(bucket == b);
            if (mask == 0ull) continue;
            const int leader = first_lane(mask);
            int got = 0;
            if (lane == leader) got = (int)atomicAdd(&c.state[b], (unsigned)__popcll(mask));
            const int64_t slot = (int64_t)(unsigned)bcast(got, leader) + mbcnt(mask);
            if (bucket == b && slot < a.P) a.tasks[(b >> 1) * a.P + ((b & 1) ? a.P - 1 - slot : slot)] = task;
        }
        loop_join();
    }
}

// ---- the distances --------------------------------------------------------------------------------------------------------------------------
// task t of the launch is tasks[t * step] (bucket 2 lies backwards)
template <int ROWS, int CPL>
__global__ __launch_bounds__(64) void mtr_k_seq_dist(SeqArgs a, const int4 *tasks, int64_t step, unsigned n_tasks)
{
    const ConsArgs &c = a.c;
    const int lane = lane_id();
    const int32_t K = a.prm.max_dist;
    if constexpr (ROWS > 1) {
        constexpr int L = 64 / ROWS;                                        // lanes of a task: a DPP row of 16, or half the wavefront
        const int r = lane & (L - 1), g = lane / L;
        const unsigned groups = (n_tasks + (unsigned)ROWS - 1u) / (unsigned)ROWS;
        for (unsigned grp = blockIdx.x; grp < groups; grp += gridDim.x) {
            const unsigned t = grp * (unsigned)ROWS + (unsigned)g;
            const bool live = t < n_tasks;                                  // (a row without a task runs the one cell of two empty windows and stores nothing)
            int32_t n = 0, m = 0; int64_t p = 0;
            const uint8_t *W = c.win_bases, *B = c.win_bases;
            if (live) {
                const int4 task = tasks[(int64_t)t * step];
                const int64_t wo = c.win_off[task.x], bo = c.win_off[task.y];
                n = (int32_t)(c.win_off[task.x + 1] - wo); m = (int32_t)(c.win_off[task.y + 1] - bo);
                W += wo; B += bo;
                p = (int64_t)(((uint64_t)(uint32_t)task.w << 32) | (uint32_t)task.z);
            }
            const BaBand band = sq_band(n, m, K);
            const int32_t last = uni(wave_max_i32(n + m));
            int32_t E = BA_INF, O = BA_INF;
            for (int32_t s = 0; s <= last; s++) {
                int32_t below, above;
                if constexpr (ROWS == 4) { below = row_shift_up1(O, BA_INF); above = row_shift_down1(E, BA_INF); }
                else {                                                      // (a wavefront shift crosses the halves' border: BA_INF is put there)
                    below = shift_up1(O, BA_INF); above = shift_down1(E, BA_INF);
                    if (r == 0) below = BA_INF;
                    if (r == L - 1) above = BA_INF;
                }
                int32_t e2 = E, o2 = O;
                sq_step(s, r, n, m, band, e2, o2, below, above, W, B);      // (past the task's last step every cell is outside the matrix: nothing is loaded)
                if (s <= n + m) { E = e2; O = o2; }
            }
            const int32_t e = sq_end_diagonal(n, m, band);
            if (live && ba_width(band) <= 2 * L && r == (e >> 1)) a.dist[p] = (uint8_t)sq_clamp((e & 1) ? O : E, K);
            loop_join();
        }
    } else {
        for (unsigned t = blockIdx.x; t < n_tasks; t += gridDim.x) {
            const int4 task = tasks[(int64_t)t * step];
            const int rt = uni(task.x), ru = uni(task.y);
            const int64_t p = (int64_t)(((uint64_t)(uint32_t)uni(task.w) << 32) | (uint32_t)uni(task.z));
            const int64_t wo = uni64(c.win_off[rt]), bo = uni64(c.win_off[ru]);
            const int32_t n = uni((int)(c.win_off[rt + 1] - wo)), m = uni((int)(c.win_off[ru + 1] - bo));
            const uint8_t *W = c.win_bases + wo, *B = c.win_bases + bo;
            const BaBand band = sq_band(n, m, K);
            if (ba_width(band) <= 128 * CPL) {
                int32_t E[CPL], O[CPL];
#pragma unroll
                for (int k = 0; k < CPL; k++) E[k] = O[k] = BA_INF;
                for (int32_t s = 0; s <= n + m; s++) {
                    int dir;
                    if (((s - band.dlo) & 1) == 0) {
                        const int32_t below = shift_up1(O[CPL - 1], BA_INF);
#pragma unroll
                        for (int k = 0; k < CPL; k++)
                            E[k] = ba_step_cell(s, 2 * (lane * CPL + k), n, m, band, E[k], O[k], k > 0 ? O[k > 0 ? k - 1 : 0] : below, W, B, dir);
                    } else {
                        const int32_t above = shift_down1(E[0], BA_INF);
#pragma unroll
                        for (int k = 0; k < CPL; k++)
                            O[k] = ba_step_cell(s, 2 * (lane * CPL + k) + 1, n, m, band, O[k], k + 1 < CPL ? E[k + 1 < CPL ? k + 1 : 0] : above, E[k], W, B, dir);
                    }
                }
                const int32_t e = sq_end_diagonal(n, m, band), pair = e >> 1;
                if (lane == pair / CPL) {
                    int32_t v = (e & 1) ? O[0] : E[0];
#pragma unroll
                    for (int k = 1; k < CPL; k++) if (pair % CPL == k) v = (e & 1) ? O[k] : E[k];
                    a.dist[p] = (uint8_t)sq_clamp(v, K);
                }
            }
            loop_join();
        }
    }
}

// ---- the split --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mtr_k_seq_split(SeqArgs a)
{
    __shared__ uint8_t mat[SQ_LDS];                                         // D(c, u) at mat[u * SQ_MAX_MEMBERS + c]
    const ConsArgs &c = a.c;
    const int lane = lane_id();
    for (int32_t l = blockIdx.x; l < c.n_loci; l += gridDim.x) {
        const int64_t e0 = uni64(c.support_off[l]);
        const int32_t S = uni((int)min((long long)(c.support_off[l + 1] - e0), (long long)SQ_MAX_MEMBERS + 1));
        SqSplit r = { 0, -1, -1, 0, 0, 0, 0 };
        if (S <= SQ_MAX_MEMBERS && S >= a.prm.min_support) {
            const uint8_t *d = a.dist + uni64(a.pair_off[l]);
            for (int32_t t = 0; t < S; t++) {
                const int64_t rs = sq_row_start(S, t);
                if (lane == 0) mat[t * SQ_MAX_MEMBERS + t] = 0;
                for (int32_t u = t + 1 + lane; u < S; u += 64) { const uint8_t v = d[rs + (u - t - 1)]; mat[u * SQ_MAX_MEMBERS + t] = v; mat[t * SQ_MAX_MEMBERS + u] = v; }
            }
            __syncthreads();
            uint32_t best = SQ_NO_KEY;
            for (int32_t m0 = lane; m0 < S; m0 += 64) { const uint32_t k = sq_cost_key(sq_cost(mat, SQ_MAX_MEMBERS, S, m0), m0); best = k < best ? k : best; }
            best = (uint32_t)uni((int)wave_min_u32(best));
            r.zygosity = 1; r.c0 = (int32_t)(best & 255u); r.cost1 = r.cost2 = (int64_t)(best >> 8); r.n0 = S;
            uint32_t key = SQ_NO_KEY;
            for (int32_t c0 = 0; c0 + 1 < S; c0++)
                for (int32_t c1 = c0 + 1 + lane; c1 < S; c1 += 64) {
                    int32_t n0, cost2;
                    sq_pair_eval(mat, SQ_MAX_MEMBERS, S, c0, c1, n0, cost2);
                    if (!sq_admissible(a.prm, S, n0, mat[c1 * SQ_MAX_MEMBERS + c0], r.cost1, cost2)) continue;
                    const uint32_t k = sq_pair_key(cost2, c0, c1);
                    key = k < key ? k : key;
                }
            key = (uint32_t)uni((int)wave_min_u32(key));
            if (key != SQ_NO_KEY) {
                r.zygosity = 2; r.c0 = (int32_t)((key >> 7) & 127u); r.c1 = (int32_t)(key & 127u); r.cost2 = (int64_t)(key >> 14);
                int32_t cost2;
                sq_pair_eval(mat, SQ_MAX_MEMBERS, S, r.c0, r.c1, r.n0, cost2);
                r.n1 = S - r.n0;
            }
        }
        // the entries: the stable partition for zygosity 2, else the list as it is (a skipped locus too, whatever its length)
        const int64_t S_all = uni64(c.support_off[l + 1]) - e0;
        int32_t before = 0;
        for (int64_t base = 0; base < S_all; base += 64) {
            const int64_t u = base + lane;
            const bool in = u < S_all;
            const bool first = in && (r.zygosity < 2 || sq_in_first(mat, SQ_MAX_MEMBERS, r.c0, r.c1, (int32_t)u));
            const unsigned long long mask = __ballot(first);
            if (in) {
                const int64_t to = e0 + (r.zygosity < 2 ? u : (int64_t)sq_place(r, (int32_t)u, first, before + mbcnt(mask)));
                a.o_value[to] = a.value[e0 + u]; a.o_read[to] = c.sup_read[e0 + u];
                a.o_allele[to] = r.zygosity == 2 && !first ? 1 : 0;
                a.o_dtm[to] = r.zygosity == 0 ? 0 : (int32_t)mat[(int32_t)u * SQ_MAX_MEMBERS + (first ? r.c0 : r.c1)];
            }
            before += (int32_t)__popcll(mask);
        }
        if (lane == 0) {
            const int32_t x0 = r.c0, x1 = r.zygosity == 2 ? r.c1 : r.c0;       // zygosity 1 names its one medoid twice in call
            a.o_zyg[l] = (uint8_t)r.zygosity;
            a.o_call[2 * l] = r.zygosity ? a.value[e0 + x0] : 0; a.o_call[2 * l + 1] = r.zygosity ? a.value[e0 + x1] : 0;
            a.o_medoid[2 * l] = r.zygosity ? c.sup_read[e0 + x0] : -1; a.o_medoid[2 * l + 1] = r.zygosity == 2 ? c.sup_read[e0 + x1] : -1;
            a.o_sup[2 * l] = r.n0; a.o_sup[2 * l + 1] = r.n1;
            a.o_cost[2 * l] = r.cost1; a.o_cost[2 * l + 1] = r.cost2;
        }
        __syncthreads();                                                    // (the matrix is read to the end before the next locus' overwrites it)
    }
}
