// genotype_quality.hip.inc — genotype quality (mtr_genotype_quality_device): every supporting read's oriented window scored against both allele
// sequences of its locus by an alignment whose costs are the read's qualities, and the scores reduced to genotype likelihoods.  The definition
// is include/mtr_hip.h's ("genotype quality"); the cell, the one-thread fill, T and the locus' reduction are genotype_quality.h, shared with the
// host; the band, the schedule and the weights are banded_align.h's.  The lists are the consensus' kernels as they are (mtr_k_cons_check,
// mtr_k_cons_members).  Every result is an exact integer and none depends on the order in which the device worked: the only atomics hand out task
// slots, and a task carries the place of its result.
//   mtr_k_gq_check       one lane per allele index: cons_off ascending from 0 to n_cons (the smallest offender is left in the state)
//   mtr_k_gq_tasks       one lane per (entry, allele): -1 where the allele does not exist or the entry is not scored, else a task of its band's
//                        bucket, the slots handed out one atomic per wavefront and bucket (mtr_k_seq_tasks' way)
//   mtr_k_gq_score<ROWS, CPL>  THE HOT PATH, mtr_k_seq_dist's schedule with int32 cells whose costs come from the read base's weight: nothing stored
//                        per cell, no scratch, no LDS.  <4, 1>: four tasks per wavefront, one per 16-lane DPP row (bands of up to 32 diagonals);
//                        <2, 1>: two, one per half (up to 64); <1, 1> and <1, 2>: one per wavefront, one or two pairs of diagonals per lane (up
//                        to 128 and 256).  The three costs of a cell are derived in the step from two quality bytes (genotype_quality.h says why)
//   mtr_k_gq_locus       one wavefront per locus: best and margin per entry, the three int64 sums by a wavefront reduction over turns of 64 entries,
//                        then pl, gt, gq by lane 0
#pragma once
#include "seq_calls.hip.inc"
#include "genotype_quality.h"

#define GQ_BLOCK 256
#define GQ_BAD_CONS 6               // the state's bad-input word of cons_off (0 .. 4 are the consensus' own)
#define GQ_MAX_GRID (1 << 16)

struct GqArgs {
    ConsArgs c;                                                         // the rows, the windows, the support lists; ent_row [S], bad, state
    const uint8_t *win_qual;                                            // [n_bases] or NULL
    const int64_t *cons_off; const uint8_t *cons_bases; int64_t n_cons; // [2 * n_loci + 1], [n_cons]
    GqParams prm;
    int4 *tasks;                                                        // [4 S]: entry row, allele index, the score's place.  With P = 2 S: bucket 0 from tasks up, 1 from tasks + P - 1 down, 2 from tasks + P up, 3 from tasks + 2 P - 1 down
    int32_t *score; uint8_t *best; int32_t *margin;                     // [S, 2], [S], [S]
    int64_t *raw, *pl; uint8_t *gt; int64_t *gq; int32_t *scored, *unscored;      // per locus
};

// ---- the lists --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GQ_BLOCK) void mtr_k_gq_check(GqArgs a)
{
    const int64_t A = (int64_t)blockIdx.x * GQ_BLOCK + threadIdx.x, G = 2 * (int64_t)a.c.n_loci;
    if (A >= G) return;
    const int64_t o0 = a.cons_off[A], o1 = a.cons_off[A + 1];
    if (o0 < 0 || o1 < o0 || o1 > a.n_cons || (A == 0 && o0 != 0) || (A == G - 1 && o1 != a.n_cons)) atomicMin(&a.c.bad[GQ_BAD_CONS], (unsigned long long)A);
}

__global__ __launch_bounds__(GQ_BLOCK) void mtr_k_gq_tasks(GqArgs a)
{
    const ConsArgs &c = a.c;
    const int lane = lane_id();
    const int64_t P = 2 * c.S;
    for (int64_t first = (int64_t)blockIdx.x * GQ_BLOCK + (threadIdx.x & ~63u); first < P; first += (int64_t)gridDim.x * GQ_BLOCK) {    // (the same for a wavefront's lanes)
        const int64_t x = first + lane;
        int bucket = -1;
        int4 task = make_int4(0, 0, 0, 0);
        if (x < P) {
            const int64_t e = x >> 1; const int al = (int)(x & 1);
            const int32_t l = cons_locus(c, e);
            const int z = c.zygosity[l];
            const int32_t row = c.ent_row[e];
            const int64_t n = c.win_off[row + 1] - c.win_off[row];
            bool scored = z > al;
            int64_t m = 0;
            for (int k = 0; k < z; k++) {                                   // scored against every existing allele, or against none
                const int64_t mk = a.cons_off[2 * (int64_t)l + k + 1] - a.cons_off[2 * (int64_t)l + k];
                if (ba_skipped(n, mk, a.prm.band_extra)) scored = false;
                if (k == al) m = mk;
            }
            if (!scored) a.score[x] = -1;
            else {
                bucket = sq_bucket(ba_width(ba_band((int32_t)n, (int32_t)m, a.prm.band_extra)));
                task = make_int4(row, 2 * l + al, (int)(uint32_t)x, 0);
            }
        }
        for (int b = 0; b < SQ_BUCKETS; b++) {
            const unsigned long long mask = __ballot(bucket == b);
            if (mask == 0ull) continue;
            const int leader = first_lane(mask);
            int got = 0;
            if (lane == leader) got = (int)atomicAdd(&c.state[b], (unsigned)__popcll(mask));
            const int64_t slot = (int64_t)(unsigned)bcast(got, leader) + mbcnt(mask);
            if (bucket == b && slot < P) a.tasks[(b >> 1) * P + ((b & 1) ? P - 1 - slot : slot)] = task;
        }
        loop_join();
    }
}

// ---- the scores -------------------------------------------------------------------------------------------------------------------------------
// task t of the launch is tasks[t * step] (buckets 1 and 3 lie backwards)
template <int ROWS, int CPL>
__global__ __launch_bounds__(64) void mtr_k_gq_score(GqArgs a, const int4 *tasks, int64_t step, unsigned n_tasks)
{
    const ConsArgs &c = a.c;
    const int lane = lane_id();
    const GqParams prm = a.prm;
    if constexpr (ROWS > 1) {
        constexpr int L = 64 / ROWS;                                        // lanes of a task: a DPP row of 16, or half the wavefront
        const int r = lane & (L - 1), g = lane / L;
        const unsigned groups = (n_tasks + (unsigned)ROWS - 1u) / (unsigned)ROWS;
        for (unsigned grp = blockIdx.x; grp < groups; grp += gridDim.x) {
            const unsigned t = grp * (unsigned)ROWS + (unsigned)g;
            const bool live = t < n_tasks;                                  // (a row without a task runs the one cell of two empty sequences and stores nothing)
            int32_t n = 0, m = 0; uint32_t place = 0;
            const uint8_t *W = c.win_bases, *Q = nullptr, *C = a.cons_bases;
            if (live) {
                const int4 task = tasks[(int64_t)t * step];
                const int64_t wo = c.win_off[task.x], co = a.cons_off[task.y];
                n = (int32_t)(c.win_off[task.x + 1] - wo); m = (int32_t)(a.cons_off[task.y + 1] - co);
                W += wo; C += co;
                if (a.win_qual) Q = a.win_qual + wo;
                place = (uint32_t)task.z;
            }
            const BaBand band = ba_band(n, m, prm.band_extra);
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
                gq_step(s, r, n, m, band, e2, o2, below, above, W, Q, C, prm);      // (past the task's last step every cell is outside the matrix: nothing is loaded)
                if (s <= n + m) { E = e2; O = o2; }
            }
            const int32_t e = gq_end_diagonal(n, m, band);
            static_assert(2 * L == (ROWS == 4 ? SQ_ROW_BAND : SQ_HALF_BAND), "a bucket's widest band is what the shape's lanes hold");
            const bool fits = ba_width(band) <= 2 * L;                      // (the task kernel's buckets say so; a task that did not fit would be left unscored, not unwritten)
            if (live && (fits ? r == (e >> 1) : r == 0)) a.score[place] = !fits ? -1 : (e & 1) ? O : E;
            loop_join();
        }
    } else {
        for (unsigned t = blockIdx.x; t < n_tasks; t += gridDim.x) {
            const int4 task = tasks[(int64_t)t * step];
            const int row = uni(task.x), A = uni(task.y);
            const uint32_t place = (uint32_t)uni(task.z);
            const int64_t wo = uni64(c.win_off[row]), co = uni64(a.cons_off[A]);
            const int32_t n = uni((int)(c.win_off[row + 1] - wo)), m = uni((int)(a.cons_off[A + 1] - co));
            const uint8_t *W = c.win_bases + wo, *Q = a.win_qual ? a.win_qual + wo : nullptr, *C = a.cons_bases + co;
            const BaBand band = ba_band(n, m, prm.band_extra);
            if (ba_width(band) <= 128 * CPL) {
                int32_t E[CPL], O[CPL];
#pragma unroll
                for (int k = 0; k < CPL; k++) E[k] = O[k] = BA_INF;
                for (int32_t s = 0; s <= n + m; s++) {
                    const int32_t neighbour = ((s - band.dlo) & 1) == 0 ? shift_up1(O[CPL - 1], BA_INF) : shift_down1(E[0], BA_INF);
                    gq_step_lane<CPL>(s, lane, n, m, band, E, O, neighbour, W, Q, C, prm);
                }
                const int32_t e = gq_end_diagonal(n, m, band), pair = e >> 1;
                if (lane == pair / CPL) {
                    int32_t v = (e & 1) ? O[0] : E[0];
#pragma unroll
                    for (int k = 1; k < CPL; k++) if (pair % CPL == k) v = (e & 1) ? O[k] : E[k];
                    a.score[place] = v;
                }
            } else if (lane == 0) a.score[place] = -1;                      // (unreachable while the task kernel's buckets and the host's shapes agree: unscored, not unwritten)
            loop_join();
        }
    }
}

// ---- the loci -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mtr_k_gq_locus(GqArgs a)
{
    const ConsArgs &c = a.c;
    const int lane = lane_id();
    for (int32_t l = blockIdx.x; l < c.n_loci; l += gridDim.x) {
        const int64_t e0 = uni64(c.support_off[l]), e1 = uni64(c.support_off[l + 1]);
        const int z = uni((int)c.zygosity[l]);
        GqSums t = { 0, 0, 0, 0, 0 };
        for (int64_t base = e0; base < e1; base += 64) {
            const int64_t e = base + lane;
            if (e < e1) {
                const int32_t s0 = a.score[2 * e], s1 = a.score[2 * e + 1];
                uint8_t best; int32_t margin;
                gq_entry(z, s0, s1, c.sup_allele[e], best, margin);
                a.best[e] = best; a.margin[e] = margin;
                gq_add(t, z, s0, s1, a.prm.read_cap);
            }
        }
        t.r0 = wave_sum_i64(t.r0); t.rh = wave_sum_i64(t.rh); t.r1 = wave_sum_i64(t.r1);
        t.scored = (int32_t)wave_sum_i64(t.scored); t.unscored = (int32_t)wave_sum_i64(t.unscored);
        if (lane == 0) {
            int64_t raw[3], pl[3], gq; uint8_t gt;
            gq_finish(z, t, raw, pl, gt, gq);
            for (int k = 0; k < 3; k++) { a.raw[3 * (int64_t)l + k] = raw[k]; a.pl[3 * (int64_t)l + k] = pl[k]; }
            a.gt[l] = gt; a.gq[l] = gq; a.scored[l] = t.scored; a.unscored[l] = t.unscored;
        }
    }
}
